// Matrix-core metric kernel (included by rmhmc_metric_mfma.hip, which sets HTA_PHILOX_MAD64 first): the dense products on zero-padded [DP][LD]
// LDS buffers as MFMA tiles - fp32 macro tiles, the bfloat16 strips and pre-split planes of the fast solve, and the out-of-line lds_gemm.
#pragma once
#include "rmhmc_metric_dev.hpp"

namespace hta {

// The phase functions are real calls (s_swappc): inlined, the trajectory kernel's body no longer fits the instruction cache a
// lone workgroup per CU has to itself and its register allocation degrades (the A/B against the all-inlined variant is recorded in
// profiles/r06e_metric_inline_ab.txt).
#define HTA_PH_ATTR __attribute__((noinline))


typedef float f4 __attribute__((ext_vector_type(4)));

// tile index -> (I, J), I <= J, row-major over the upper block triangle
__device__ __forceinline__ void upper_tile(int t, int nt, int& I, int& J) {
  I = 0;
  while (t >= nt - I) { t -= nt - I; ++I; }
  J = I + t;
}

// C = Cinit + op(A) op(B) on zero-padded [DP][LD] buffers.  op(A)[m][k] = TA ? A[k][m] : A[m][k]; op(B)[k][n] = TB ? B[n][k]
// : B[k][n], times kscale[k] when SCALE.  SYM: the product is symmetric - upper macro tiles only, mirrored on store.
// Lane l of a wave feeds A[m = l & 15][k = l >> 4], B[k = l >> 4][n = l & 15] and owns C[4 (l >> 4) + r][l & 15].
//
// A wave owns one MACRO tile of 2 x 2 instruction tiles: an operand fetched from LDS feeds two instructions (LDS traffic is
// what bounds a one-tile-per-wave loop: 2 x 256 bytes per 32-cycle instruction and SIMD) and the four accumulators are
// independent chains (40 cycles of dependent latency against 32 of issue).  nt <= 7 gives at most 16 macro tiles, one per
// wave; they are dealt out by size (full 2 x 2 tiles, then the 1 x 2 / 2 x 1 edges of an odd nt, then the corner) in
// boustrophedon order over the four SIMDs - wave w runs on SIMD w & 3 - so that the matrix pipes get equal shares.
// The contraction covers k4 steps of four indices (k4 = ceil(D / 4)): chunks of four steps, the operands of the next chunk
// in flight while the current one is on the pipe; the steps beyond the last full chunk take indices 4 ks + lk.
// the k loop of one macro tile; R2 / C2: the macro tile has a second tile row / column
template <bool TA, bool TB, bool SCALE, bool R2, bool C2>
__device__ __forceinline__ void gemm_macro(const float* pa0, const float* pb0, const float* kscale, int k4, int LD, int lk, f4 (&acc)[2][2]) {
  const int as = TA ? 4 * LD : 4, bs = TB ? 4 : 4 * LD;
  const float* pa1 = pa0 + (TA ? 16 : 16 * LD);
  const float* pb1 = pb0 + (TB ? 16 * LD : 16);
  float av[2][2][4], bv[2][2][4];                               // [buffer][tile row / column][step]
  float scv[2][4];                                              // the chunk's scale factors: applied where the operand is consumed (applied
                                                                // where it is loaded, the multiply - and with it the wait for the NEXT chunk's reads -
                                                                // sits in front of the CURRENT chunk's matrix instructions: no read was ever in flight)
#define HTA_LOAD_STEP(buf, u, ks)                                                        \
  do {                                                                                   \
    av[buf][0][u] = pa0[(ks) * as];                                                      \
    if (R2) av[buf][1][u] = pa1[(ks) * as];                                              \
    const float sc__ = SCALE ? kscale[4 * (ks) + lk] : 1.f;                              \
    bv[buf][0][u] = SCALE ? pb0[(ks) * bs] * sc__ : pb0[(ks) * bs];                      \
    if (C2) bv[buf][1][u] = SCALE ? pb1[(ks) * bs] * sc__ : pb1[(ks) * bs];              \
    scv[buf][u] = 1.f;                                                                   \
  } while (0)
#define HTA_MMA_STEP(buf, u)                                                                                              \
  do {                                                                                                                    \
    const float b0__ = SCALE ? bv[buf][0][u] * scv[buf][u] : bv[buf][0][u];                                               \
    const float b1__ = (SCALE && C2) ? bv[buf][1][u] * scv[buf][u] : bv[buf][1][u];                                       \
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[buf][0][u], b0__, acc[0][0], 0, 0, 0);                            \
    if (C2) acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[buf][0][u], b1__, acc[0][1], 0, 0, 0);                    \
    if (R2) acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[buf][1][u], b0__, acc[1][0], 0, 0, 0);                    \
    if (R2 && C2) acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[buf][1][u], b1__, acc[1][1], 0, 0, 0);              \
  } while (0)
  // A chunk = 16 contraction indices = four instructions.  Inside a chunk, lane group lk takes the indices 16 c + 4 lk + u at
  // step u (not 16 c + 4 u + lk: any assignment serves as long as both operands use it): an operand that is contiguous
  // in k (A[m][k], B[n][k], the scale vector) arrives as ONE 16-byte read per chunk, and an operand that is strided in k
  // (A[k][m], B[k][n]) is read from rows 4 lk + u - with LD = 4 mod 8 the four lane groups of an instruction fall on four
  // different bank quarters.  (Rounds 2-3 read rows 4 u + lk: groups 0 / 1 of LD = 116 overlapped in four banks, and the
  // k-contiguous operand took four 4-byte reads with rows li and li + 8 in the same banks: every operand read of every
  // product was a two-way bank conflict, and LDS time - not the matrix pipe - bounded the products.)
  const float* qa0 = pa0 + (TA ? 3 * lk * LD : 3 * lk);
  const float* qa1 = pa1 + (TA ? 3 * lk * LD : 3 * lk);
  const float* qb0 = pb0 + (TB ? 3 * lk : 3 * lk * LD);
  const float* qb1 = pb1 + (TB ? 3 * lk : 3 * lk * LD);
  const float* qsc = SCALE ? kscale + 4 * lk : nullptr;
#define HTA_LOAD_CHUNK(buf, c)                                                                                            \
  do {                                                                                                                    \
    if (TA) {                                                                                                             \
      _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                                     \
        av[buf][0][u] = qa0[(16 * (c) + u) * LD];                                                                         \
        if (R2) av[buf][1][u] = qa1[(16 * (c) + u) * LD];                                                                 \
      }                                                                                                                   \
    } else {                                                                                                              \
      const f4 t0__ = *reinterpret_cast<const f4*>(qa0 + 16 * (c));                                                       \
      _Pragma("unroll") for (int u = 0; u < 4; ++u) av[buf][0][u] = t0__[u];                                              \
      if (R2) {                                                                                                           \
        const f4 t1__ = *reinterpret_cast<const f4*>(qa1 + 16 * (c));                                                     \
        _Pragma("unroll") for (int u = 0; u < 4; ++u) av[buf][1][u] = t1__[u];                                            \
      }                                                                                                                   \
    }                                                                                                                     \
    if (SCALE) {                                                                                                          \
      const f4 sc__ = *reinterpret_cast<const f4*>(qsc + 16 * (c));                                                       \
      _Pragma("unroll") for (int u = 0; u < 4; ++u) scv[buf][u] = sc__[u];                                                \
    }                                                                                                                     \
    if (TB) {                                                                                                             \
      const f4 t0__ = *reinterpret_cast<const f4*>(qb0 + 16 * (c));                                                       \
      _Pragma("unroll") for (int u = 0; u < 4; ++u) bv[buf][0][u] = t0__[u];                                              \
      if (C2) {                                                                                                           \
        const f4 t1__ = *reinterpret_cast<const f4*>(qb1 + 16 * (c));                                                     \
        _Pragma("unroll") for (int u = 0; u < 4; ++u) bv[buf][1][u] = t1__[u];                                            \
      }                                                                                                                   \
    } else {                                                                                                              \
      _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                                     \
        bv[buf][0][u] = qb0[(16 * (c) + u) * LD];                                                                         \
        if (C2) bv[buf][1][u] = qb1[(16 * (c) + u) * LD];                                                                 \
      }                                                                                                                   \
    }                                                                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
  } while (0)
  const int nchunk = k4 >> 2;
  if (nchunk > 0) {
    HTA_LOAD_CHUNK(0, 0);
    int ch = 0;
    for (; ch + 2 < nchunk; ch += 2) {
      HTA_LOAD_CHUNK(1, ch + 1);
#pragma unroll
      for (int u = 0; u < 4; ++u) HTA_MMA_STEP(0, u);
      __builtin_amdgcn_sched_barrier(0);
      HTA_LOAD_CHUNK(0, ch + 2);
#pragma unroll
      for (int u = 0; u < 4; ++u) HTA_MMA_STEP(1, u);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (ch + 1 < nchunk) {
      HTA_LOAD_CHUNK(1, ch + 1);
#pragma unroll
      for (int u = 0; u < 4; ++u) HTA_MMA_STEP(0, u);
#pragma unroll
      for (int u = 0; u < 4; ++u) HTA_MMA_STEP(1, u);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) HTA_MMA_STEP(0, u);
    }
  }
  for (int ks = 4 * nchunk; ks < k4; ++ks) {
    HTA_LOAD_STEP(0, 0, ks);
    HTA_MMA_STEP(0, 0);
  }
#undef HTA_LOAD_STEP
#undef HTA_LOAD_CHUNK
#undef HTA_MMA_STEP
}

// The same macro tile for M = F E1 with the operands split on the fly into two bfloat16 terms each (x = hi + lo + O(2^-16 x)) and three
// products on v_mfma_f32_16x16x32_bf16 (hi hi + hi lo + lo hi, fp32 accumulation): 48 cycles of the matrix pipe per 32 contraction
// indices instead of 256.  M is a second-order CORRECTION - |E2| = |M| / gap <= 1e-4 where this pass is taken (kSecondE) - so its
// relative error 2^-16 is an absolute error below 2e-9 in the eigenvectors: under fp32 rounding of the first-order terms, which stay
// exact fp32 products (formation, and every matrix-vector product of the solve).  Both operands are read along k: A = F[m][k]
// (symmetric), B = E1[k][n] = -E1[n][k] (antisymmetric: the caller negates the result); lane l feeds row / column l & 15 and the
// indices 8 (l >> 4) .. + 7 of a 32-step (16-byte reads, rows 464 bytes apart: conflict free), 4 (l >> 4) .. + 3 of the 16-step that
// ends an odd number of tiles.
typedef __bf16 bf8v __attribute__((ext_vector_type(8)));
typedef short s4v __attribute__((ext_vector_type(4)));
typedef int i4v __attribute__((ext_vector_type(4)));
typedef int i2v __attribute__((ext_vector_type(2)));
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split_pair(float x0, float x1, int& hi, int& lo) {
  const unsigned a = __float_as_uint(x0), b = __float_as_uint(x1);
  hi = (int)__builtin_amdgcn_perm(b, a, 0x07060302);                     // the upper halves: truncation to bfloat16
  const f2v x = {x0, x1}, h = {__uint_as_float(a & 0xffff0000u), __uint_as_float(b & 0xffff0000u)};
  const f2v r = x - h;
  lo = (int)__builtin_amdgcn_perm(__float_as_uint(r[1]), __float_as_uint(r[0]), 0x07060302);
}
// (F arrives already split: the formation's epilogue stores it as two bfloat16 planes [DP][DP] (hi, then lo; rows 2 DP bytes apart - with an odd
// tile count the 16 lanes of a ds_read_b128 group fall on 16 different quads of the bank row) in the buffer fp32 F would take.  Measured
// (builds with the matrix instructions or the operand reads compiled out: profiles/r06i_metric_fast_phases.txt): a k loop's time is the SUM of its matrix instructions' time and its other instructions' time, not the larger -
// every split saved is time saved.)
// A 1 x NB strip of the second product: ONE tile of E1 rows (operand A, fp32, split on the fly ONCE per 32 indices) against NB <= 4 tiles
// of F's planes (operand B) - the 2 x 2 macro tile split its two A tiles for two B tiles each, and the split is what that loop's time is
// made of.  acc[y] = sum_k E1[j][k] F[i_y][k] = -M[i_y][j].
// NT: the tile count as a compile-time constant (the planes exist only where the leading dimension is kLdCfg3, i.e. 7 tiles): the k loop
// unrolls completely - every operand read is an immediate offset of ONE address register per operand and the next step's A tile lands in
// fresh registers (the rolled loop spent 18 address additions and 4 register-pair copies per step next to its 12 matrix instructions).
template <int NB, int NT>
__device__ __forceinline__ void gemm_strip_bx3(const float* pa0, const unsigned short* pb0, f4 (&acc)[4]) {
  constexpr int nt = NT;
  const int kg = (threadIdx.x & 63) >> 4;
  constexpr int DPh = 16 * nt, plane = DPh * DPh;
  const float* pa = pa0 + 8 * kg;
  const unsigned short* pb = pb0 + 8 * kg;
  constexpr int nfull = nt >> 1;
  f4 ra0, ra1;
  if (nfull > 0) { ra0 = *reinterpret_cast<const f4*>(pa); ra1 = *reinterpret_cast<const f4*>(pa + 4); }
#pragma unroll
  for (int s = 0; s < nfull; ++s) {
    // (B tiles two at a time: all four at once put the function beyond the caller-saved registers)
    i4v bh[2], bl[2];
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      if (y >= NB) continue;
      bh[y] = *reinterpret_cast<const i4v*>(pb + y * 16 * DPh + 32 * s);
      bl[y] = *reinterpret_cast<const i4v*>(pb + y * 16 * DPh + plane + 32 * s);
    }
    i4v ah, al;
    {
      int h, l;
      split_pair(ra0[0], ra0[1], h, l); ah[0] = h; al[0] = l;
      split_pair(ra0[2], ra0[3], h, l); ah[1] = h; al[1] = l;
      split_pair(ra1[0], ra1[1], h, l); ah[2] = h; al[2] = l;
      split_pair(ra1[2], ra1[3], h, l); ah[3] = h; al[3] = l;
    }
    __builtin_amdgcn_sched_barrier(0);
    if (s + 1 < nfull) { ra0 = *reinterpret_cast<const f4*>(pa + 32 * (s + 1)); ra1 = *reinterpret_cast<const f4*>(pa + 32 * (s + 1) + 4); }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int pr = 0; pr < 3; ++pr)
#pragma unroll
      for (int y = 0; y < 2; ++y) {
        if (y >= NB) continue;
        acc[y] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8v, pr == 2 ? al : ah), __builtin_bit_cast(bf8v, pr == 1 ? bl[y] : bh[y]), acc[y], 0, 0, 0);
      }
    __builtin_amdgcn_sched_barrier(0);
    if (NB > 2) {
#pragma unroll
      for (int y = 2; y < 4; ++y) {
        if (y >= NB) continue;
        bh[y - 2] = *reinterpret_cast<const i4v*>(pb + y * 16 * DPh + 32 * s);
        bl[y - 2] = *reinterpret_cast<const i4v*>(pb + y * 16 * DPh + plane + 32 * s);
      }
#pragma unroll
      for (int pr = 0; pr < 3; ++pr)
#pragma unroll
        for (int y = 2; y < 4; ++y) {
          if (y >= NB) continue;
          acc[y] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8v, pr == 2 ? al : ah), __builtin_bit_cast(bf8v, pr == 1 ? bl[y - 2] : bh[y - 2]), acc[y], 0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (nt & 1) {
    const int k0 = 16 * (nt - 1) + 4 * kg - 8 * kg;
    const f4 v = *reinterpret_cast<const f4*>(pa + k0);
    i2v th, tl;
    { int h, l; split_pair(v[0], v[1], h, l); th[0] = h; tl[0] = l; split_pair(v[2], v[3], h, l); th[1] = h; tl[1] = l; }
#pragma unroll
    for (int y = 0; y < NB; ++y) {
      const i2v uh = *reinterpret_cast<const i2v*>(pb + y * 16 * DPh + k0), ul = *reinterpret_cast<const i2v*>(pb + y * 16 * DPh + plane + k0);
      acc[y] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s4v, th), __builtin_bit_cast(s4v, uh), acc[y], 0, 0, 0);
      acc[y] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s4v, th), __builtin_bit_cast(s4v, ul), acc[y], 0, 0, 0);
      acc[y] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s4v, tl), __builtin_bit_cast(s4v, uh), acc[y], 0, 0, 0);
    }
  }
}

// Both operands pre-split (the formation F = W W^T on the planes of W^T = (diag(sqrt e) V0)^T, round 6): a row tile against one or two
// row tiles, three products per tile and 32 indices, no vector instruction in the loop.  pa / pb: row starts of the hi plane.
template <bool C2, int NT>
__device__ __forceinline__ void gemm_macro_pp(const unsigned short* pa0, const unsigned short* pb0, f4 (&acc)[2][2]) {
  constexpr int nt = NT;                                                  // (compile-time tile count: see gemm_strip_bx3)
  const int kg = (threadIdx.x & 63) >> 4;
  constexpr int DPh = 16 * nt, plane = DPh * DPh;
  const unsigned short* pa = pa0 + 8 * kg;
  const unsigned short* pb[2] = {pb0 + 8 * kg, pb0 + 16 * DPh + 8 * kg};
  constexpr int nfull = nt >> 1;
  i4v ah, al, bh[2], bl[2];
#define HTA_PP_LOAD(s)                                                                                   \
  do {                                                                                                   \
    ah = *reinterpret_cast<const i4v*>(pa + 32 * (s)); al = *reinterpret_cast<const i4v*>(pa + plane + 32 * (s)); \
    bh[0] = *reinterpret_cast<const i4v*>(pb[0] + 32 * (s)); bl[0] = *reinterpret_cast<const i4v*>(pb[0] + plane + 32 * (s)); \
    if (C2) { bh[1] = *reinterpret_cast<const i4v*>(pb[1] + 32 * (s)); bl[1] = *reinterpret_cast<const i4v*>(pb[1] + plane + 32 * (s)); } \
  } while (0)
  if (nfull > 0) HTA_PP_LOAD(0);
#pragma unroll
  for (int s = 0; s < nfull; ++s) {
    const i4v cah = ah, cal = al, cbh0 = bh[0], cbl0 = bl[0], cbh1 = bh[1], cbl1 = bl[1];
    __builtin_amdgcn_sched_barrier(0);
    if (s + 1 < nfull) HTA_PP_LOAD(s + 1);
    __builtin_amdgcn_sched_barrier(0);
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8v, cah), __builtin_bit_cast(bf8v, cbh0), acc[0][0], 0, 0, 0);
    if (C2) acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8v, cah), __builtin_bit_cast(bf8v, cbh1), acc[0][1], 0, 0, 0);
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8v, cah), __builtin_bit_cast(bf8v, cbl0), acc[0][0], 0, 0, 0);
    if (C2) acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8v, cah), __builtin_bit_cast(bf8v, cbl1), acc[0][1], 0, 0, 0);
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8v, cal), __builtin_bit_cast(bf8v, cbh0), acc[0][0], 0, 0, 0);
    if (C2) acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8v, cal), __builtin_bit_cast(bf8v, cbh1), acc[0][1], 0, 0, 0);
  }
#undef HTA_PP_LOAD
  if (nt & 1) {                                                          // the last 16 indices
    const int k0 = 16 * (nt - 1) + 4 * kg - 8 * kg;
    const i2v th = *reinterpret_cast<const i2v*>(pa + k0), tl = *reinterpret_cast<const i2v*>(pa + plane + k0);
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      if (y == 1 && !C2) continue;
      const i2v uh = *reinterpret_cast<const i2v*>(pb[y] + k0), ul = *reinterpret_cast<const i2v*>(pb[y] + plane + k0);
      acc[0][y] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s4v, th), __builtin_bit_cast(s4v, uh), acc[0][y], 0, 0, 0);
      acc[0][y] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s4v, th), __builtin_bit_cast(s4v, ul), acc[0][y], 0, 0, 0);
      acc[0][y] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s4v, tl), __builtin_bit_cast(s4v, uh), acc[0][y], 0, 0, 0);
    }
  }
}

// (Operands are OFFSETS, in floats, into the kernel's dynamic LDS block: an out-of-line function only sees generic pointers
// in its arguments - flat loads, every wait a full one; and its integer arguments arrive in vector registers: readfirstlane
// makes them scalars again so that the tile bookkeeping compiles to scalar branches.)
// LDC: the leading dimension as a compile-time constant (0: the run-time value) - with it the four rows of a chunk's operand
// reads are immediate offsets of one address register instead of an address computation per read
template <bool TA, bool TB, bool SYM, bool SCALE, int LDC>
__device__ HTA_PH_ATTR void lds_gemm_ld(int offA, int offB, int offC, int offCinit, int offScale, int nt, int k4, int LDr) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* const lds = reinterpret_cast<float*>(smem_raw);
  nt = __builtin_amdgcn_readfirstlane(nt); k4 = __builtin_amdgcn_readfirstlane(k4);
  const int LD = LDC ? LDC : __builtin_amdgcn_readfirstlane(LDr);
  const float* A = lds + __builtin_amdgcn_readfirstlane(offA);
  const float* B = lds + __builtin_amdgcn_readfirstlane(offB);
  float* C = lds + __builtin_amdgcn_readfirstlane(offC);
  offCinit = __builtin_amdgcn_readfirstlane(offCinit);
  const float* Cinit = offCinit >= 0 ? lds + offCinit : nullptr;
  const float* kscale = SCALE ? lds + __builtin_amdgcn_readfirstlane(offScale) : nullptr;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);        // wave-uniform: scalar branches below
  const int li = lane & 15, lk = lane >> 4;
  int I0, J0;
  bool r2, c2;
  if (SYM) {
    // upper block triangle only, as 1 x 2 macro tiles (pairs of neighbours in a tile row) and the odd tile that ends a row of odd
    // length: nt = 7 gives 12 pairs + 4 singles = one item per wave, pairs first - every SIMD (wave & 3) gets three pairs and a
    // single, 7 of the 28 tiles.  (Round 3 dealt 2 x 2 macro tiles here too: 10 items for 16 waves, three full ones - 12 tiles -
    // on one SIMD: a symmetric product took as long as a full one.)
    int npairs = 0;
    for (int I = 0; I < nt; ++I) npairs += (nt - I) >> 1;
    int w = wave, I = 0;
    if (w < npairs) {
      for (;; ++I) { const int pr = (nt - I) >> 1; if (w < pr) break; w -= pr; }
      I0 = I; J0 = I + 2 * w; c2 = true;
    } else {
      w -= npairs;
      for (; I < nt; ++I) if ((nt - I) & 1) { if (w == 0) break; --w; }
      if (I >= nt) return;
      I0 = I; J0 = nt - 1; c2 = false;
    }
    r2 = false;
  } else {
    const int nf = nt >> 1, odd = nt & 1;
    const int s = wave & 3, q = wave >> 2;
    int k = (q & 1) ? 4 * q + 3 - s : 4 * q + s;                  // position in the size-sorted macro list
    int r, c;
    const int nfull = nf * nf;
    if (k < nfull) { r = k / nf; c = k - r * nf; }
    else {
      k -= nfull;
      if (!odd || k > 2 * nf) return;
      if (k < nf) { r = k; c = nf; } else if (k < 2 * nf) { r = nf; c = k - nf; } else { r = nf; c = nf; }
    }
    I0 = 2 * r; J0 = 2 * c;
    r2 = I0 + 1 < nt; c2 = J0 + 1 < nt;
  }
  const float* pa0 = TA ? A + lk * LD + 16 * I0 + li : A + (16 * I0 + li) * LD + lk;
  const float* pb0 = TB ? B + (16 * J0 + li) * LD + lk : B + lk * LD + 16 * J0 + li;
  f4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      acc[x][y] = f4{0.f, 0.f, 0.f, 0.f};
      if (Cinit && (x == 0 || r2) && (y == 0 || c2)) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[x][y][t] = Cinit[(16 * (I0 + x) + 4 * lk + t) * LD + 16 * (J0 + y) + li];
      }
    }
  if (r2 && c2) gemm_macro<TA, TB, SCALE, true, true>(pa0, pb0, kscale, k4, LD, lk, acc);
  else if (r2) gemm_macro<TA, TB, SCALE, true, false>(pa0, pb0, kscale, k4, LD, lk, acc);
  else if (c2) gemm_macro<TA, TB, SCALE, false, true>(pa0, pb0, kscale, k4, LD, lk, acc);
  else gemm_macro<TA, TB, SCALE, false, false>(pa0, pb0, kscale, k4, LD, lk, acc);
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      if ((x == 1 && !r2) || (y == 1 && !c2)) continue;
      const int I = I0 + x, J = J0 + y;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        C[(16 * I + 4 * lk + t) * LD + 16 * J + li] = acc[x][y][t];
        if (SYM && I != J) C[(16 * J + li) * LD + 16 * I + 4 * lk + t] = acc[x][y][t];
      }
    }
}

constexpr int kLdCfg3 = 116;             // LD of 97 <= D <= 112 (BASELINE config 3's D = 100)
constexpr int kNtCfg3 = (kLdCfg3 - 4) / 16;      // its tile count: 7
template <bool TA, bool TB, bool SYM, bool SCALE>
__device__ __forceinline__ void lds_gemm(int offA, int offB, int offC, int offCinit, int offScale, int nt, int k4, int LD) {
  if (LD == kLdCfg3) lds_gemm_ld<TA, TB, SYM, SCALE, kLdCfg3>(offA, offB, offC, offCinit, offScale, nt, k4, LD);
  else lds_gemm_ld<TA, TB, SYM, SCALE, 0>(offA, offB, offC, offCinit, offScale, nt, k4, LD);
}

}  // namespace hta
