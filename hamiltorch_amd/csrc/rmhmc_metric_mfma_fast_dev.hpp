// Matrix-core metric kernel: the LDS layout (MetricLds), the fast solve of a Gaussian target on the shared basis (metric_fast_solve, its
// ph_fast_* phases, the packed resident entries) and the trajectory kernel's resident state (ph_res_out / res_in).
#pragma once
#include "rmhmc_metric_mfma_phases_dev.hpp"

namespace hta {

// ======== Round 6: the SOLVE evaluation of a Gaussian target on the shared basis - 4 L + 2 of a trajectory's 4 L + 3 =============
// Same mathematics as the general sequence in metric_warm_system (formation, first pass from X = I, second pass in closed form applied
// to the vectors), reorganised around what the phase table of round 5 showed (profiles/r05ad: 71 k cycles, of which the two
// products' k loops are 19.5 k): (1) V0 never leaves its buffer - X = I + E1 is not stored over it, E1 and E2 live in the other two,
// so nothing is staged again (3.0 k + the first staging); (2) the element-wise passes run in the EPILOGUES of the two products on
// the accumulators (no LDS round trip of S / M, no pair bookkeeping, 16-byte mirror stores: 6.5 k + 8.0 k -> ~4 k); (3) log p and
// P d come from the eigenbasis the workgroup already holds - d' = V0^T d rides in the pass that computes m' = V0^T m, d^T P d =
// sum lam0 d'^2, P d = V0 (lam0 d') rides in the pass that computes x = V0 x' - instead of a pass over P in global memory with an
// L2 read-modify-write behind it (8.3 k -> ~2 k); (4) the three block sums (log-det, quadratic form, d^T P d) share the chain's
// barriers.  Anything this path does not cover (per-system curvature, outputs that need G or Q, a first pass above kSecondE, a second
// pass above kConvE) returns false BEFORE any global write and the general sequence runs, V0 still resident.
constexpr int kFastScratch = 320 + 4 * 112;   // floats at oW: the Cholesky's [16][20] panel scratch (the fast solve parks its [10][4] wave partials there), then the
                                              // trajectory kernel's four state vectors in eigen-coordinates (kFastState: theta', p', theta~', p~', DP floats each)
constexpr int kFastState = 320;

// The workgroup's dynamic LDS block, in floats, for the padded dimension DP and the leading dimension LD - the ONE statement of it, for
// both sequences, the trajectory kernel and the host launchers:
//   three matrix buffers of BS floats | DP-float vectors e, lam, lam~, m, y, x, then d (2 DP) | MT / 64 reduction slots | kFastScratch
// (the fast solve keeps (m_i, d_i) pairs in y | x and calls the scratch's head oS; the phases address the vectors as oVec + k DP, oVec = oJit).
// The members are computed in the order and the form (a chain of additions) in which metric_warm_system used to write them out: the
// generated code of the general sequence follows that, not only the values.
struct MetricLds {
  int DP;
  int BS;         // floats per matrix buffer (gmv_sym parks 8 x 128 slice partials in one: at least 1024)
  int oB1, oB2;   // the second and third matrix buffer (the first is at 0)
  int oJit;       // e = jitter * u                          (later: Jacobi (c, s) pairs)
  int oLam;       // eigenvalues of Hs
  int oLt;        // soft-abs eigenvalues
  int oM;         // m, then m' = V0^T m
  int oY;         // w = (X^T m') / lam~
  int oX;         // x' = X w
  int oD;         // d = X - mu / z
  int oRed;       // MT / 64
  int oW;         // [16][20] panel scratch; the fast solve's wave partials (its oS)
  int oSt;        // the resident trajectory's theta', p', theta~', p~': state(0 .. 3)
  int floats;     // the whole block
  __host__ __device__ __forceinline__ constexpr MetricLds(int dp, int ld)
      : DP(dp), BS(dp * ld > 1024 ? dp * ld : 1024), oB1(BS), oB2(2 * BS), oJit(3 * BS), oLam(oJit + dp), oLt(oLam + dp), oM(oLt + dp), oY(oM + dp), oX(oY + dp), oD(oX + dp),
        oRed(oD + 2 * dp), oW(oRed + MT / 64), oSt(oW + kFastState), floats(oW + kFastScratch) {}
  __host__ __device__ __forceinline__ constexpr int buf(int k) const { return k * BS; }
  __host__ __device__ __forceinline__ constexpr int state(int k) const { return oSt + k * DP; }
};

// What the trajectory kernel and traj_general_eval address: MetricLds's oY and its four resident state vectors, written in closed form (the
// generated code of those two functions follows the shape of this arithmetic, not only its value).  The assertion ties it to MetricLds.
struct TrajLds {
  int BS, oY, oSt, sTh, sP, sThc, sPc;       // sTh .. sPc: theta', p', theta~', p~'
  __host__ __device__ __forceinline__ constexpr TrajLds(int DP, int LD)
      : BS(DP * LD > 1024 ? DP * LD : 1024), oY(3 * BS + 4 * DP), oSt(3 * BS + 8 * DP + MT / 64 + kFastState), sTh(oSt), sP(oSt + DP), sThc(oSt + 2 * DP), sPc(oSt + 3 * DP) {}
};
constexpr bool traj_lds_agrees(int DP, int LD) {
  const MetricLds m(DP, LD);
  const TrajLds t(DP, LD);
  return t.BS == m.BS && t.oY == m.oY && t.sTh == m.state(0) && t.sP == m.state(1) && t.sThc == m.state(2) && t.sPc == m.state(3) && t.sPc + DP <= m.floats;
}
static_assert(traj_lds_agrees(16, 20) && traj_lds_agrees(64, 68) && traj_lds_agrees(112, 116), "TrajLds restates MetricLds");

// ph_fast_chain's `flags`
constexpr int kChainSkip2 = 1;       // no second pass (E2 = 0)
constexpr int kChainHasX = 2;        // log p / P d wanted
constexpr int kChainResident = 4;    // the state lives in LDS in eigen-coordinates (the trajectory kernel)
constexpr int kChainDraw = 8;        // the DRAW p = G^(1/2) z: w = y sqrt(lam~) instead of y / lam~
constexpr int kChainAssign = 16;     // (with kChainResident) x' REPLACES the resident vector, no second update
constexpr int kChainStrips = 32;     // the second product ran on strips (two partial vectors)
constexpr int kChainMapped = 64;     // ... and its idle waves took the soft-abs map (no first barrier in the chain)
// The packed argument of the resident entries (ph_fast_form_r / ph_fast_second_strip_r / ph_fast_chain_r; see ResLayout): V0's buffer index
// in bits 0 .. 1, D in bits 2 .. 9, the chain's flags from bit 10.
constexpr int kResBufMask = 3, kResDShift = 2, kResDMask = 255, kResFlagShift = 10;
__device__ __forceinline__ int res_code(int vb, int D) { return vb | (D << kResDShift); }

// Cost model of the vector phases (measured, round 6: profiles/r06i_metric_fast_phases.txt): with 16 waves on the CU every instruction a
// wave executes costs the workgroup ~16 cycles (4 waves per SIMD x 4 cycles of issue; the ONE scalar unit of the CU serves all 16 waves),
// whatever it does - a matrix-vector product spread over all 1024 threads is bound by its address / predicate / reduction instructions,
// not by its 12.5 k multiply-adds.  So these phases run on the first 8 waves only, 4 lanes per row with 32 multiply-adds each as packed
// FMAs; the other waves go straight to the next barrier.  Lane c of a row takes the 16-byte quads 4c .. 4c+3 and 16+4c .. 16+4c+3: the 16
// lanes of a ds_read_b128 group (4 rows x 4 lanes, rows 29 quads apart) then fall on 16 different quads of the bank row.
__device__ __forceinline__ f2v pk_fma(f2v a, f2v b, f2v c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float quad_sum(float s) { s += dpp_f<0xB1>(s); s += dpp_f<0x4E>(s); return s; }

// (M v)_row, row = tid >> 2, tid < 512; nq = quads per row (DP / 4, a multiple of 4); every lane of the row's quad returns the sum
__device__ __forceinline__ float mv4(const float* M, int ld, const float* v, int nq, int nrow) {
  const int row = threadIdx.x >> 2, c = threadIdx.x & 3;
  f2v a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
  if (row < nrow) {
    const float* mr = M + row * ld + 16 * c;
    const float* vr = v + 16 * c;
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) {
      if (16 * rd + 4 * c < nq) {
        f4 mq[4], vq[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) { mq[t] = *reinterpret_cast<const f4*>(mr + 64 * rd + 4 * t); vq[t] = *reinterpret_cast<const f4*>(vr + 64 * rd + 4 * t); }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          a0 = pk_fma(f2v{mq[t][0], mq[t][1]}, f2v{vq[t][0], vq[t][1]}, a0);
          a1 = pk_fma(f2v{mq[t][2], mq[t][3]}, f2v{vq[t][2], vq[t][3]}, a1);
        }
      }
    }
  }
  return quad_sum((a0[0] + a0[1]) + (a1[0] + a1[1]));
}

// two products on one pass over M: (M v0, M v1)
__device__ __forceinline__ void mv4_dual(const float* M, int ld, const float* v0, const float* v1, int nq, int nrow, float& o0, float& o1) {
  const int row = threadIdx.x >> 2, c = threadIdx.x & 3;
  f2v a0 = {0.f, 0.f}, a1 = {0.f, 0.f}, b0 = {0.f, 0.f}, b1 = {0.f, 0.f};
  if (row < nrow) {
    const float* mr = M + row * ld + 16 * c;
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) {
      if (16 * rd + 4 * c < nq) {
        f4 mq[4], xq[4], yq[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          mq[t] = *reinterpret_cast<const f4*>(mr + 64 * rd + 4 * t);
          xq[t] = *reinterpret_cast<const f4*>(v0 + 16 * c + 64 * rd + 4 * t);
          yq[t] = *reinterpret_cast<const f4*>(v1 + 16 * c + 64 * rd + 4 * t);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          a0 = pk_fma(f2v{mq[t][0], mq[t][1]}, f2v{xq[t][0], xq[t][1]}, a0);
          a1 = pk_fma(f2v{mq[t][2], mq[t][3]}, f2v{xq[t][2], xq[t][3]}, a1);
          b0 = pk_fma(f2v{mq[t][0], mq[t][1]}, f2v{yq[t][0], yq[t][1]}, b0);
          b1 = pk_fma(f2v{mq[t][2], mq[t][3]}, f2v{yq[t][2], yq[t][3]}, b1);
        }
      }
    }
  }
  o0 = quad_sum((a0[0] + a0[1]) + (a1[0] + a1[1]));
  o1 = quad_sum((b0[0] + b0[1]) + (b1[0] + b1[1]));
}

// (M^T v)_k, k = tid >> 2, tid < 512: lane c sums the rows 4u + c (4-byte reads along the row: the 32 lanes of a read group touch
// 4 banks twice); nrow = DP (a multiple of 16).  Every lane of the column's quad returns the sum.
__device__ __forceinline__ float mv4t(const float* M, int ld, const float* v, int nrow) {
  const int k = threadIdx.x >> 2, c = threadIdx.x & 3;
  float a0 = 0.f, a1 = 0.f;
  if (k < nrow) {
    const float* mc = M + c * ld + k;
    const float* vc = v + c;
    for (int u0 = 0; 4 * u0 < nrow; u0 += 8) {                     // rows 4 (u0 + t) + c, eight (or four: nrow / 4 is a multiple of 4) in flight
      float mv[8], vv[8];
      const bool two = 4 * (u0 + 4) < nrow;
#pragma unroll
      for (int t = 0; t < 4; ++t) { mv[t] = mc[4 * (u0 + t) * ld]; vv[t] = vc[4 * (u0 + t)]; }
      if (two) {
#pragma unroll
        for (int t = 4; t < 8; ++t) { mv[t] = mc[4 * (u0 + t) * ld]; vv[t] = vc[4 * (u0 + t)]; }
      } else {
#pragma unroll
        for (int t = 4; t < 8; ++t) { mv[t] = 0.f; vv[t] = 0.f; }
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) { if (t & 1) a1 = fmaf(mv[t], vv[t], a1); else a0 = fmaf(mv[t], vv[t], a0); }
    }
  }
  return quad_sum(a0 + a1);
}

// m' = V0^T m and d' = V0^T d in one pass over V0 (mv4t's layout, (m_i, d_i) interleaved at offMD), waves 0 .. 7
__device__ HTA_PH_ATTR void ph_fast_vt(int offV, int offMD, int offM, int offD, int DP, int LD) {
  HTA_LDS_BASE();
  DP = HTA_U(DP); LD = HTA_U(LD);
  if (threadIdx.x < 512) {
    const float* V = lds + HTA_U(offV);
    const f2v* md = reinterpret_cast<const f2v*>(lds + HTA_U(offMD));
    const int k = threadIdx.x >> 2, c = threadIdx.x & 3;
    f2v a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
    if (k < DP) {
      const float* mc = V + c * LD + k;
      for (int u0 = 0; 4 * u0 < DP; u0 += 8) {
        float mv[8]; f2v w[8];
        const bool two = 4 * (u0 + 4) < DP;
#pragma unroll
        for (int t = 0; t < 4; ++t) { mv[t] = mc[4 * (u0 + t) * LD]; w[t] = md[4 * (u0 + t) + c]; }
        if (two) {
#pragma unroll
          for (int t = 4; t < 8; ++t) { mv[t] = mc[4 * (u0 + t) * LD]; w[t] = md[4 * (u0 + t) + c]; }
        } else {
#pragma unroll
          for (int t = 4; t < 8; ++t) { mv[t] = 0.f; w[t] = f2v{0.f, 0.f}; }
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) { if (t & 1) a1 = pk_fma(f2v{mv[t], mv[t]}, w[t], a1); else a0 = pk_fma(f2v{mv[t], mv[t]}, w[t], a0); }
      }
    }
    const float sm = quad_sum(a0[0] + a1[0]), sd = quad_sum(a0[1] + a1[1]);
    if (c == 0 && k < DP) { (lds + HTA_U(offM))[k] = sm; (lds + HTA_U(offD))[k] = sd; }
  }
  __syncthreads();
}

// The work items of the two products, once per launch (the scalar loops that deal them out cost every wave ~100 instructions per call
// on the CU's one scalar unit: the waves entered their k loops 1 .. 3.4 k cycles apart).  Bits 0 .. 9: the wave's item of the upper block
// triangle as lds_gemm_ld's SYM branch deals them (I0 | J0 << 4 | second tile << 8 | active << 9); bits 16 .. 26: its 2 x 2 macro tile
// of a full product as the other branch does (I0 | J0 << 4 | second row << 8 | second column << 9 | active << 10).
__device__ __forceinline__ int fast_tiles(int nt) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int lo, hi;
  {
    int npairs = 0;
    for (int I = 0; I < nt; ++I) npairs += (nt - I) >> 1;
    int w = wave, I = 0, I0, J0, c2 = 0, active = 1;
    if (w < npairs) {
      for (;; ++I) { const int pr = (nt - I) >> 1; if (w < pr) break; w -= pr; }
      I0 = I; J0 = I + 2 * w; c2 = 1;
    } else {
      w -= npairs;
      for (; I < nt; ++I) if ((nt - I) & 1) { if (w == 0) break; --w; }
      if (I >= nt) { active = 0; I = 0; }
      I0 = I; J0 = nt - 1;
    }
    lo = I0 | (J0 << 4) | (c2 << 8) | (active << 9);
  }
  {
    const int nf = nt >> 1, odd = nt & 1;
    const int s = wave & 3, q = wave >> 2;
    int k = (q & 1) ? 4 * q + 3 - s : 4 * q + s;
    int r = 0, c = 0, active = 1;
    const int nfull = nf * nf;
    if (k < nfull) { r = k / nf; c = k - r * nf; }
    else {
      k -= nfull;
      if (!odd || k > 2 * nf) active = 0;
      else if (k < nf) { r = k; c = nf; } else if (k < 2 * nf) { r = nf; c = k - nf; } else { r = nf; c = nf; }
    }
    const int I0 = 2 * r, J0 = 2 * c;
    hi = I0 | (J0 << 4) | ((I0 + 1 < nt ? 1 : 0) << 8) | ((J0 + 1 < nt ? 1 : 0) << 9) | (active << 10);
  }
  // bits 27 .. 30 / 31: the wave's STRIP of the second product's bfloat16 form (ph_fast_second_strip) and whether it has one.  Strip s < nt:
  // column tile J = s against row tiles 0 .. 3; strip nt + J: against row tiles 4 .. nt - 1.  nt = 7 (BASELINE config 3): 7 strips of four
  // tiles and 7 of three dealt so that the four SIMDs (wave & 3) carry 13 / 12 / 12 / 12 tiles.
  int sid = wave, sact = wave < nt * ((nt + 3) >> 2) ? 1 : 0;
  if (nt == 7) {
    const int big[7] = {0, 1, 5, 9, 2, 6, 10}, small[7] = {4, 8, 12, 3, 7, 11, 15};
    sact = 0;
    for (int k = 0; k < 7; ++k) { if (wave == big[k]) { sid = k; sact = 1; } if (wave == small[k]) { sid = 7 + k; sact = 1; } }
  }
  return (int)((unsigned)(lo | (hi << 16)) | ((unsigned)(sid & 15) << 27) | ((unsigned)sact << 31));
}

// F as two bfloat16 planes (PL: what the bfloat16 form of the second product reads): hi = the upper half of the fp32 word, lo = the upper
// half of (x - hi); a lane's four values are four ROWS of the tile (2-byte stores) and four consecutive columns of its mirror image (8 bytes)
__device__ __forceinline__ void plane_store_col(unsigned short* ph, unsigned short* pl, int stride, const f4& a) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const unsigned b = __float_as_uint(a[t]);
    const float r = a[t] - __uint_as_float(b & 0xffff0000u);
    ph[t * stride] = (unsigned short)(b >> 16);
    pl[t * stride] = (unsigned short)(__float_as_uint(r) >> 16);
  }
}
__device__ __forceinline__ void plane_store_row(unsigned short* ph, unsigned short* pl, const f4& a) {
  int h0, l0, h1, l1;
  split_pair(a[0], a[1], h0, l0); split_pair(a[2], a[3], h1, l1);
  *reinterpret_cast<i2v*>(ph) = i2v{h0, h1};
  *reinterpret_cast<i2v*>(pl) = i2v{l0, l1};
}

// F = V0^T diag(e) V0 (upper tiles, as lds_gemm_ld<true, false, true, true>) with the first pass in the epilogue: the diagonal tiles
// publish lam_i = lam0_i + F_ii, then every tile turns its accumulators into E1_ij = F_ij / (lam_j - lam_i) (ph_refine_E's
// arithmetic with X = I: the same quotients, the same threshold) and stores F (zero diagonal) and E1 (antisymmetric, zero
// diagonal) with their mirror images as 16-byte rows.  Returns max |E1_ij| (1 for NaN / inf / > kFallbackE).
// WB (round 6, "metric_bx3" = 2): the formation itself on bfloat16.  W^T = (diag(sqrt e) V0)^T is written once per evaluation as two bfloat16
// planes (hi, lo) into E1's buffer - idle until the epilogue - by a pass that reads V0 column-wise (4-byte reads, consecutive lanes on
// consecutive columns) and stores 16-byte groups of eight contraction indices; F = W^T W is then three products per tile and 32 indices
// with NO vector instruction in the loop (gemm_macro_pp): 1.2 k cycles of the matrix pipe per SIMD instead of 5.6 k.  Each term of F carries a
// relative error 2^-16; emulated in float64 around it (tools/scratch/bf16_formation_err.py), max |x - x64| / max |x64| of a solve moves from
// 7.4e-8 to 7.8e-8 at BASELINE config 3's jitter (1.5e-7 to 1.9e-7 at three times the jitter) - the closed-form second pass's own truncation
// is that size, the kernel's fp32 vector arithmetic (3.6e-6) is fifty times it.
template <int LDC, bool PL, bool WB = false>
__device__ __forceinline__ float fast_form_body(int offV, int offF, int offE, int offJit, int offLam0, int offLam, int offRed, int tile, int k4, int D, int LDr, int nt) {
  HTA_LDS_BASE();
  k4 = HTA_U(k4); D = HTA_U(D); nt = LDC == kLdCfg3 ? kNtCfg3 : HTA_U(nt);
  const int LD = LDC ? LDC : HTA_U(LDr);
  const float* V = lds + HTA_U(offV);
  float* F = lds + HTA_U(offF); float* E = lds + HTA_U(offE);
  const float* kscale = lds + HTA_U(offJit);
  const float* vlam0 = lds + HTA_U(offLam0);
  float* vlam = lds + HTA_U(offLam); float* red = lds + HTA_U(offRed);
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lk = lane >> 4;
  tile = HTA_U(tile);                                              // fast_tiles(): this wave's item of the upper block triangle
  const int I0 = tile & 15, J0 = (tile >> 4) & 15;
  const bool c2 = (tile >> 8) & 1, active = (tile >> 9) & 1;
  f4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = f4{0.f, 0.f, 0.f, 0.f};
  if (WB) {
    // W^T planes: thread (column i = tid & 127 of V0, octet o = tid >> 7 [+ 8]) scales V0[8 o .. 8 o + 7][i] by sqrt(e) and splits
    unsigned short* Wh = reinterpret_cast<unsigned short*>(E);
    const int DPh = 16 * nt, plane = DPh * DPh;
    const int i = threadIdx.x & 127, o0 = HTA_U(threadIdx.x >> 7);
    if (i < DPh) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int o = o0 + 8 * u;
        if (8 * o < DPh) {
          float w[8];
          const f4 s0 = *reinterpret_cast<const f4*>(kscale + 8 * o), s1 = *reinterpret_cast<const f4*>(kscale + 8 * o + 4);
#pragma unroll
          for (int r = 0; r < 8; ++r) w[r] = V[(8 * o + r) * LD + i] * (r < 4 ? s0[r] : s1[r - 4]);      // (the scale vector holds sqrt(e) here: metric_fast_solve)
          int h[4], l[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) split_pair(w[2 * r], w[2 * r + 1], h[r], l[r]);
          *reinterpret_cast<i4v*>(Wh + i * DPh + 8 * o) = i4v{h[0], h[1], h[2], h[3]};
          *reinterpret_cast<i4v*>(Wh + plane + i * DPh + 8 * o) = i4v{l[0], l[1], l[2], l[3]};
        }
      }
    }
    __syncthreads();
  }
  if (active) {
    if (WB) {
      const unsigned short* Wh = reinterpret_cast<const unsigned short*>(E);
      const unsigned short* pa0 = Wh + (16 * I0 + li) * (16 * nt);
      const unsigned short* pb0 = Wh + (16 * J0 + li) * (16 * nt);
      if (c2) gemm_macro_pp<true, kNtCfg3>(pa0, pb0, acc); else gemm_macro_pp<false, kNtCfg3>(pa0, pb0, acc);
    } else {
      const float* pa0 = V + lk * LD + 16 * I0 + li;
      const float* pb0 = V + lk * LD + 16 * J0 + li;
      if (c2) gemm_macro<true, false, true, false, true>(pa0, pb0, kscale, k4, LD, lk, acc);
      else gemm_macro<true, false, true, false, false>(pa0, pb0, kscale, k4, LD, lk, acc);
    }
    if (I0 == J0) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (4 * lk + t == li) { const int i = 16 * I0 + li; if (i < D) vlam[i] = acc[0][0][t] + vlam0[i]; }
    }
  }
  __syncthreads();
  const float sc = wave_max_abs(vlam, 16 * nt);                     // (entries D .. DP - 1 of lam are zero)
  const float tiny = 8.f * Eps<float>::v * sc;
  unsigned ebits = 0u;                                             // max |E1_ij| as a bit pattern: inf and NaN order above every finite value
  if (active) {
    const f4 lamI = *reinterpret_cast<const f4*>(vlam + 16 * I0 + 4 * lk);
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      if (y == 1 && !c2) continue;
      const int J = J0 + y, j = 16 * J + li;
      const float lamJ = vlam[j];
      if (I0 != J) {
        const f4 a = acc[0][y];
        const f2v lamJ2 = {lamJ, lamJ};
        const f2v d01 = lamJ2 - f2v{lamI[0], lamI[1]}, d23 = lamJ2 - f2v{lamI[2], lamI[3]};
        const f2v r01 = {__builtin_amdgcn_rcpf(d01[0]), __builtin_amdgcn_rcpf(d01[1])}, r23 = {__builtin_amdgcn_rcpf(d23[0]), __builtin_amdgcn_rcpf(d23[1])};
        const f2v q01 = f2v{a[0], a[1]} * r01, q23 = f2v{a[2], a[3]} * r23;
        f4 e;
        e[0] = (fabsf(a[0]) <= tiny) ? 0.f : q01[0];
        e[1] = (fabsf(a[1]) <= tiny) ? 0.f : q01[1];
        e[2] = (fabsf(a[2]) <= tiny) ? 0.f : q23[0];
        e[3] = (fabsf(a[3]) <= tiny) ? 0.f : q23[1];
        float* fd = F + (16 * I0 + 4 * lk) * LD + j;
        float* ed = E + (16 * I0 + 4 * lk) * LD + j;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          ebits = max(ebits, __float_as_uint(e[t]) & 0x7fffffffu);
          if (!PL) fd[t * LD] = a[t];
          ed[t * LD] = e[t];
        }
        const f2v n01 = f2v{e[0], e[1]} * f2v{-1.f, -1.f}, n23 = f2v{e[2], e[3]} * f2v{-1.f, -1.f};
        if (PL) {
          unsigned short* Fh = reinterpret_cast<unsigned short*>(F);
          const int DPh = 16 * nt, plane = DPh * DPh;
          plane_store_col(Fh + (16 * I0 + 4 * lk) * DPh + j, Fh + plane + (16 * I0 + 4 * lk) * DPh + j, DPh, a);
          plane_store_row(Fh + j * DPh + 16 * I0 + 4 * lk, Fh + plane + j * DPh + 16 * I0 + 4 * lk, a);
        } else {
          *reinterpret_cast<f4*>(F + j * LD + 16 * I0 + 4 * lk) = a;
        }
        *reinterpret_cast<f4*>(E + j * LD + 16 * I0 + 4 * lk) = f4{n01[0], n01[1], n23[0], n23[1]};
      } else {
        // a diagonal tile holds both triangles of its block: every lane stores its own four elements, no mirror.  (F_ij and F_ji differ
        // in the last bit there - the scale factor enters through the B operand only - so E1 + E1^T is zero to rounding of a 5e-3
        // quantity, not exactly: 1e-10, far below anything the solve resolves.)
        const f4 a = acc[0][y];
        const f2v lamJ2 = {lamJ, lamJ};
        const f2v d01 = lamJ2 - f2v{lamI[0], lamI[1]}, d23 = lamJ2 - f2v{lamI[2], lamI[3]};
        const f2v r01 = {__builtin_amdgcn_rcpf(d01[0]), __builtin_amdgcn_rcpf(d01[1])}, r23 = {__builtin_amdgcn_rcpf(d23[0]), __builtin_amdgcn_rcpf(d23[1])};
        const f2v q01 = f2v{a[0], a[1]} * r01, q23 = f2v{a[2], a[3]} * r23;
        f4 e;
        e[0] = (fabsf(a[0]) <= tiny) ? 0.f : q01[0];
        e[1] = (fabsf(a[1]) <= tiny) ? 0.f : q01[1];
        e[2] = (fabsf(a[2]) <= tiny) ? 0.f : q23[0];
        e[3] = (fabsf(a[3]) <= tiny) ? 0.f : q23[1];
        float* fd = F + (16 * I0 + 4 * lk) * LD + j;
        float* ed = E + (16 * I0 + 4 * lk) * LD + j;
        f4 f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const bool dg = 4 * lk + t == li;
          e[t] = dg ? 0.f : e[t]; f[t] = dg ? 0.f : a[t];
          ebits = max(ebits, __float_as_uint(e[t]) & 0x7fffffffu);
          if (!PL) fd[t * LD] = f[t];
          ed[t * LD] = e[t];
        }
        if (PL) {
          unsigned short* Fh = reinterpret_cast<unsigned short*>(F);
          const int DPh = 16 * nt, plane = DPh * DPh;
          plane_store_col(Fh + (16 * I0 + 4 * lk) * DPh + j, Fh + plane + (16 * I0 + 4 * lk) * DPh + j, DPh, f);
        }
      }
    }
  }
  float emax = (ebits > __float_as_uint(kFallbackE)) ? 1.f : __uint_as_float(ebits);      // NaN / inf / too large
  emax = block_max1(emax, red);         // (`red` was last read before this function's barrier above)
  return emax;
}
template <int LDC, bool PL, bool WB = false>
__device__ HTA_PH_ATTR float ph_fast_form(int offV, int offF, int offE, int offJit, int offLam0, int offLam, int offRed, int tile, int k4, int D, int LDr, int nt) {
  return fast_form_body<LDC, PL, WB>(offV, offF, offE, offJit, offLam0, offLam, offRed, tile, k4, D, LDr, nt);
}
// The RESIDENT evaluations of the trajectory kernel at kLdCfg3 (ph_fast_form_r / ph_fast_second_strip_r / ph_fast_chain_r): every LDS offset
// is a compile-time function of the buffer V0 sits in (MetricLds at that dimension), so a call passes ONE packed word (res_code(), the chain's
// flags above it) instead of 12 ... 21 registers - an argument costs the caller a move (often a read of a parked scalar as well) and the
// callee a readfirstlane, per wave, and with 16 waves on the CU every one of those is ~16 cycles: ~1 k cycles per call.
struct ResLayout {
  int bx, by, bz, oJit, oLam, oLt, oRed, D;
  __device__ __forceinline__ explicit ResLayout(int code) {
    constexpr MetricLds m(16 * kNtCfg3, kLdCfg3);
    code = HTA_U(code);
    const int vb = code & kResBufMask;
    bx = m.buf(vb); by = vb == 0 ? m.buf(1) : m.buf(0); bz = vb == 2 ? m.buf(1) : m.buf(2);
    oJit = m.oJit; oLam = m.oLam; oLt = m.oLt; oRed = m.oRed;
    D = (code >> kResDShift) & kResDMask;
  }
};
__device__ HTA_PH_ATTR float ph_fast_form_r(int code, int tile) {
  const ResLayout r(code);
  return fast_form_body<kLdCfg3, true, true>(r.bx, r.by, r.bz, r.oJit, r.oLt, r.oLam, r.oRed, tile, (r.D + 3) >> 2, r.D, kLdCfg3, kNtCfg3);
}

// M = F E1 (as lds_gemm_ld<false, false, false, false>) with the closed-form second pass in the epilogue (ph_refine_E2's arithmetic
// on the accumulators): lam_i' = lam_i + M_ii from the diagonal tiles, E2_ij = M_ij / (lam_j' - lam_i'), E2_ii = -1/2 sum_k E1_ik^2
// (row sums taken before the product), E2 stored over F once every wave has left its k loop.  Returns max |E2_ij|.
template <int LDC>
// Round 6, later: the vectors' first two products ride along.  The pass over E1 that takes the row sums also takes E1 m' - y0 = m' - E1 m'
// is published before the product - and the epilogue, which holds E2 in registers, accumulates y0^T E2 per column (a DPP row sum over the 16
// rows of a tile, one 16-byte store of four columns per tile and lane group) into one partial vector per macro-tile row (offP0 .. offP3:
// idle vectors); the chain starts from y = y0 + the sum of those partials instead of two matrix-vector products and a barrier.
__device__ HTA_PH_ATTR float ph_fast_second(int offF, int offE, int oVec, int offRed, int nt, int tile, int k4, int D, int LDr) {
  HTA_LDS_BASE();
  nt = HTA_U(nt); k4 = HTA_U(k4); D = HTA_U(D); oVec = HTA_U(oVec);
  const int LD = LDC ? LDC : HTA_U(LDr);
  const int DPv = 16 * nt;
  float* F = lds + HTA_U(offF); const float* E = lds + HTA_U(offE);
  float* vlam = lds + oVec + DPv; const float* vm = lds + oVec + 3 * DPv; float* vy = lds + oVec + 4 * DPv; float* vcs = lds + oVec + 7 * DPv;
  float* red = lds + HTA_U(offRed);
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lk = lane >> 4;
  {
    const int row = threadIdx.x >> 3, seg = threadIdx.x & 7;
    float c0 = 0.f, c1 = 0.f, u0 = 0.f, u1 = 0.f;
    if (row < 16 * nt) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = seg + 8 * u;
        if (q < 4 * nt) {
          const f4 v = *reinterpret_cast<const f4*>(E + row * LD + 4 * q);
          const f4 mq = *reinterpret_cast<const f4*>(vm + 4 * q);
          // (packed: the same sums in the same order, half the instructions)
          const f2v v01 = {v[0], v[1]}, v23 = {v[2], v[3]};
          f2v cc = pk_fma(v01, v01, f2v{c0, c1}); cc = pk_fma(v23, v23, cc); c0 = cc[0]; c1 = cc[1];
          f2v uu = pk_fma(v01, f2v{mq[0], mq[1]}, f2v{u0, u1}); uu = pk_fma(v23, f2v{mq[2], mq[3]}, uu); u0 = uu[0]; u1 = uu[1];
        }
      }
    }
    const float cs = sum8_dpp(c0 + c1), e1m = sum8_dpp(u0 + u1);
    if (seg == 0 && row < 16 * nt) { vcs[row] = cs; vy[row] = (row < D) ? vm[row] - e1m : 0.f; }
  }
  tile = HTA_U(tile) >> 16;                                        // fast_tiles(): this wave's 2 x 2 macro tile of the full product
  const int I0 = tile & 15, J0 = (tile >> 4) & 15;
  const bool r2 = (tile >> 8) & 1, c2 = (tile >> 9) & 1, active = (tile >> 10) & 1;
  // The instruction computes the TRANSPOSED tile: its rows run over j (operand A = rows of E1), its columns over i (operand B = rows of
  // the symmetric F), acc[x][y][t] = sum_k E1[j][k] F[i][k] = -M[i][j] at i = 16 (I0 + y) + li, j = 16 (J0 + x) + 4 lk + t - a lane
  // holds four consecutive columns of ONE row of M, so E2 leaves as one 16-byte store per tile and lane and the element-wise step runs
  // on register pairs (v_pk_add / v_pk_mul).  The sign goes into the reciprocal: E2_ij = M_ij / (lam_j - lam_i) = acc / (lam_i - lam_j).
  f4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = f4{0.f, 0.f, 0.f, 0.f};
  if (active) {
    // (exact fp32 products; the bfloat16 form runs on strips: ph_fast_second_strip)
    {
      const float* pa0 = E + (16 * J0 + li) * LD + lk;
      const float* pb0 = F + lk * LD + 16 * I0 + li;
      if (r2 && c2) gemm_macro<false, false, false, true, true>(pa0, pb0, nullptr, k4, LD, lk, acc);
      else if (c2) gemm_macro<false, false, false, true, false>(pa0, pb0, nullptr, k4, LD, lk, acc);
      else if (r2) gemm_macro<false, false, false, false, true>(pa0, pb0, nullptr, k4, LD, lk, acc);
      else gemm_macro<false, false, false, false, false>(pa0, pb0, nullptr, k4, LD, lk, acc);
    }
    if (I0 == J0) {                                                // lam_i' = lam_i + M_ii
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        if (x == 1 && !r2) continue;
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (4 * lk + t == li) { const int i = 16 * (I0 + x) + li; if (i < D) vlam[i] = vlam[i] - acc[x][x][t]; }
      }
    }
  }
  __syncthreads();
  const float sc = wave_max_abs(vlam, 16 * nt);                     // (entries D .. DP - 1 of lam are zero)
  const float tiny = 8.f * Eps<float>::v * sc * kSecondE;
  unsigned ebits = 0u;                                             // max |E2_ij| as a bit pattern: inf and NaN order above every finite value
  f4 pacc[2] = {f4{0.f, 0.f, 0.f, 0.f}, f4{0.f, 0.f, 0.f, 0.f}};   // y0^T E2 over this wave's rows, per column tile
  if (active) {
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      if (y == 1 && !r2) continue;
      const int I = I0 + y, i = 16 * I + li;
      const float lamI = vlam[i], y0i = vy[i];
      const f2v lamI2 = {lamI, lamI};
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        if (x == 1 && !c2) continue;
        const int J = J0 + x;
        const f4 lamJ = *reinterpret_cast<const f4*>(vlam + 16 * J + 4 * lk);
        const f4 a = acc[x][y];
        const f2v d01 = lamI2 - f2v{lamJ[0], lamJ[1]}, d23 = lamI2 - f2v{lamJ[2], lamJ[3]};
        const f2v r01 = {__builtin_amdgcn_rcpf(d01[0]), __builtin_amdgcn_rcpf(d01[1])}, r23 = {__builtin_amdgcn_rcpf(d23[0]), __builtin_amdgcn_rcpf(d23[1])};
        const f2v q01 = f2v{a[0], a[1]} * r01, q23 = f2v{a[2], a[3]} * r23;
        f4 e;
        e[0] = (fabsf(a[0]) <= tiny) ? 0.f : q01[0];
        e[1] = (fabsf(a[1]) <= tiny) ? 0.f : q01[1];
        e[2] = (fabsf(a[2]) <= tiny) ? 0.f : q23[0];
        e[3] = (fabsf(a[3]) <= tiny) ? 0.f : q23[1];
        if (I == J) {                                              // (wave-uniform) the diagonal element: E2_ii = -1/2 sum_k E1_ik^2, not an update
          const float dg = -0.5f * vcs[i];
#pragma unroll
          for (int t = 0; t < 4; ++t) if (4 * lk + t == li) e[t] = 0.f;
#pragma unroll
          for (int t = 0; t < 4; ++t) ebits = max(ebits, __float_as_uint(e[t]) & 0x7fffffffu);
#pragma unroll
          for (int t = 0; t < 4; ++t) if (4 * lk + t == li) e[t] = dg;
        } else {
#pragma unroll
          for (int t = 0; t < 4; ++t) ebits = max(ebits, __float_as_uint(e[t]) & 0x7fffffffu);
        }
        *reinterpret_cast<f4*>(F + i * LD + 16 * J + 4 * lk) = e;
#pragma unroll
        for (int t = 0; t < 4; ++t) pacc[x][t] = fmaf(e[t], y0i, pacc[x][t]);
      }
    }
    // one partial vector per macro-tile row: vectors that are idle here (e | m' | x | the Cholesky's panel scratch)
    float* part = lds + (I0 == 0 ? oVec : I0 == 2 ? oVec + 3 * DPv : I0 == 4 ? oVec + 5 * DPv : oVec + 8 * DPv + MT / 64 + 64);
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      if (x == 1 && !c2) continue;
      f4 sum;
#pragma unroll
      for (int t = 0; t < 4; ++t) sum[t] = sum16_dpp(pacc[x][t]);
      if (li == 0) *reinterpret_cast<f4*>(part + 16 * (J0 + x) + 4 * lk) = sum;
    }
  }
  float emax = (ebits > __float_as_uint(kFallbackE)) ? 1.f : __uint_as_float(ebits);      // NaN / inf / too large
  emax = block_max1(emax, red);
  return emax;
}

// The soft-abs map of rows i (one wave: 64 consecutive rows) - lam~ over lam0 at vlt, lam0 d' over d' at vd, the wave's partials of the
// log-determinant and of sum lam0 d'^2 into slot `wslot` of the block-sum table.  Runs on waves 8 .. 9 of ph_fast_chain, or (round 6, later)
// on the two waves ph_fast_second_strip leaves without a strip, under that phase's element-wise step.
__device__ __forceinline__ void fast_softabs_rows(int i, int wslot, int D, int DP, float alpha, const float* vlam, float* vlt, float* vd, float* red3,
                                                  float* lam_out, float* lamraw_out, bool has_x, bool sync_after_map) {
  typedef __attribute__((address_space(1))) float* gf;
  float ld = 0.f, lq = 0.f, lt = 1.f, l0 = 0.f;
  if (i < D) {
    const float lam = vlam[i], x = alpha * lam;
    // |alpha lam| >= 10: tanh is 1 - 4e-9, i.e. tanhf returns +-1 exactly, lam / tanh = |lam| bit for bit - the whole wave skips the function's body when
    // every eigenvalue is there (the identity soft-abs map of BASELINE config 3: alpha = 1e6)
    const bool sat = fabsf(x) >= 10.f;
    if (__builtin_amdgcn_ballot_w64(!sat) == 0) lt = fabsf(lam);
    else lt = (1.f / tanhf(x)) * lam;
    l0 = vlt[i];                                               // (lam0 is parked where lam~ goes)
    if (lamraw_out) ((gf)lamraw_out)[i] = lam;
  }
  if (i < DP) vlt[i] = lt;
  if (sync_after_map) __syncthreads();                         // (ph_fast_chain without a second pass: the first of its four barriers - y0)
  if (i < D) {
    ld = logf(lt);
    if (lam_out) ((gf)lam_out)[i] = lt;
    if (has_x) { const float dp = vd[i]; lq = l0 * dp * dp; vd[i] = l0 * dp; }
  }
  const float s0 = wave_sum_dpp(ld), s2 = wave_sum_dpp(lq);
  if ((threadIdx.x & 63) == 0) { float* r = red3 + 4 * wslot; r[0] = s0; r[1] = 0.f; r[2] = s2; }
}

// The bfloat16 form of the second product on 1 x 4 / 1 x 3 STRIPS (fast_tiles bits 27 .. 31): the same pre-pass, barrier and element-wise step
// as ph_fast_second<.., true>, one E1 tile per wave split once per 32 indices for up to four tiles of F's planes; the partial vectors of
// E2^T y0 are two (row tiles 0 .. 3 -> the slot of I0 = 0, row tiles 4 .. -> the slot of I0 = 4: ph_fast_chain's kChainStrips).
template <int LDC>
__device__ __forceinline__ float fast_second_strip_body(int offF, int offE, int oVec, int offRed, int nt, int tile, int D, float alpha, int has_x,
                                                        float* lam_out, float* lamraw_out) {
  HTA_LDS_BASE();
  static_assert(LDC == kLdCfg3, "the planes exist at this leading dimension only");
  nt = kNtCfg3; D = HTA_U(D); oVec = HTA_U(oVec);
  constexpr int LD = LDC;
  const int DPv = 16 * nt;
  float* F = lds + HTA_U(offF); const float* E = lds + HTA_U(offE);
  float* vlam = lds + oVec + DPv; const float* vm = lds + oVec + 3 * DPv; float* vy = lds + oVec + 4 * DPv; float* vcs = lds + oVec + 7 * DPv;
  float* red = lds + HTA_U(offRed);
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lk = lane >> 4;
  {
    const int row = threadIdx.x >> 3, seg = threadIdx.x & 7;
    float c0 = 0.f, c1 = 0.f, u0 = 0.f, u1 = 0.f;
    if (row < 16 * nt) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = seg + 8 * u;
        if (q < 4 * nt) {
          const f4 v = *reinterpret_cast<const f4*>(E + row * LD + 4 * q);
          const f4 mq = *reinterpret_cast<const f4*>(vm + 4 * q);
          // (packed: the same sums in the same order, half the instructions)
          const f2v v01 = {v[0], v[1]}, v23 = {v[2], v[3]};
          f2v cc = pk_fma(v01, v01, f2v{c0, c1}); cc = pk_fma(v23, v23, cc); c0 = cc[0]; c1 = cc[1];
          f2v uu = pk_fma(v01, f2v{mq[0], mq[1]}, f2v{u0, u1}); uu = pk_fma(v23, f2v{mq[2], mq[3]}, uu); u0 = uu[0]; u1 = uu[1];
        }
      }
    }
    const float cs = sum8_dpp(c0 + c1), e1m = sum8_dpp(u0 + u1);
    if (seg == 0 && row < 16 * nt) { vcs[row] = cs; vy[row] = (row < D) ? vm[row] - e1m : 0.f; }
  }
  const unsigned tl = (unsigned)HTA_U(tile);
  const int sid = (tl >> 27) & 15;
  const bool active = (tl >> 31) != 0;
  const int part = sid >= nt ? 1 : 0, J = sid - part * nt, I0 = 4 * part;
  const int cnt = part ? nt - 4 : (nt < 4 ? nt : 4);
  f4 acc[4];
#pragma unroll
  for (int y = 0; y < 4; ++y) acc[y] = f4{0.f, 0.f, 0.f, 0.f};
  if (active) {
    const float* pa0 = E + (16 * J + li) * LD;
    const unsigned short* pb0 = reinterpret_cast<const unsigned short*>(F) + (16 * I0 + li) * (16 * nt);
    if (cnt == 4) gemm_strip_bx3<4, kNtCfg3>(pa0, pb0, acc);      // (7 tiles: strips of 4 and 3)
    else gemm_strip_bx3<3, kNtCfg3>(pa0, pb0, acc);
#pragma unroll
    for (int y = 0; y < 4; ++y)
      if (y < cnt && I0 + y == J) {                                // lam_i' = lam_i + M_ii
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (4 * lk + t == li) { const int i = 16 * J + li; if (i < D) vlam[i] = vlam[i] - acc[y][t]; }
      }
  }
  __syncthreads();
  const float sc = wave_max_abs(vlam, 16 * nt);                     // (entries D .. DP - 1 of lam are zero)
  const float tiny = 8.f * Eps<float>::v * sc * kSecondE;
  unsigned ebits = 0u;
  {
    // the two waves without a strip (fast_tiles: 13 and 14 at 7 tiles) take the soft-abs map of the corrected eigenvalues, which ph_fast_chain
    // would otherwise wait for behind a barrier of its own (kChainMapped there)
    const int wv = HTA_U(threadIdx.x >> 6);
    if (wv == 13 || wv == 14)
      fast_softabs_rows((int)threadIdx.x - 13 * 64, 8 + wv - 13, D, DPv, alpha, vlam, lds + oVec + 2 * DPv, lds + oVec + 6 * DPv, lds + oVec + 8 * DPv + MT / 64,
                        lam_out, lamraw_out, HTA_U(has_x) != 0, false);
  }
  if (active) {
    const f4 lamJ = *reinterpret_cast<const f4*>(vlam + 16 * J + 4 * lk);
    f4 pacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      if (y >= cnt) continue;
      const int I = I0 + y, i = 16 * I + li;
      const float lamI = vlam[i], y0i = vy[i];
      const f2v lamI2 = {lamI, lamI};
      const f4 a = acc[y];
      const f2v d01 = lamI2 - f2v{lamJ[0], lamJ[1]}, d23 = lamI2 - f2v{lamJ[2], lamJ[3]};
      const f2v r01 = {__builtin_amdgcn_rcpf(d01[0]), __builtin_amdgcn_rcpf(d01[1])}, r23 = {__builtin_amdgcn_rcpf(d23[0]), __builtin_amdgcn_rcpf(d23[1])};
      const f2v q01 = f2v{a[0], a[1]} * r01, q23 = f2v{a[2], a[3]} * r23;
      f4 e;
      e[0] = (fabsf(a[0]) <= tiny) ? 0.f : q01[0];
      e[1] = (fabsf(a[1]) <= tiny) ? 0.f : q01[1];
      e[2] = (fabsf(a[2]) <= tiny) ? 0.f : q23[0];
      e[3] = (fabsf(a[3]) <= tiny) ? 0.f : q23[1];
      if (I == J) {
        const float dg = -0.5f * vcs[i];
#pragma unroll
        for (int t = 0; t < 4; ++t) if (4 * lk + t == li) e[t] = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) ebits = max(ebits, __float_as_uint(e[t]) & 0x7fffffffu);
#pragma unroll
        for (int t = 0; t < 4; ++t) if (4 * lk + t == li) e[t] = dg;
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) ebits = max(ebits, __float_as_uint(e[t]) & 0x7fffffffu);
      }
      *reinterpret_cast<f4*>(F + i * LD + 16 * J + 4 * lk) = e;
#pragma unroll
      for (int t = 0; t < 4; ++t) pacc[t] = fmaf(e[t], y0i, pacc[t]);
    }
    float* pv = lds + (part ? oVec + 5 * DPv : oVec);
    f4 sum;
#pragma unroll
    for (int t = 0; t < 4; ++t) sum[t] = sum16_dpp(pacc[t]);
    if (li == 0) *reinterpret_cast<f4*>(pv + 16 * J + 4 * lk) = sum;
  }
  float emax = (ebits > __float_as_uint(kFallbackE)) ? 1.f : __uint_as_float(ebits);
  emax = block_max1(emax, red);
  return emax;
}
template <int LDC>
__device__ HTA_PH_ATTR float ph_fast_second_strip(int offF, int offE, int oVec, int offRed, int nt, int tile, int D, float alpha, int has_x,
                                                  float* lam_out, float* lamraw_out) {
  return fast_second_strip_body<LDC>(offF, offE, oVec, offRed, nt, tile, D, alpha, has_x, lam_out, lamraw_out);
}
__device__ HTA_PH_ATTR float ph_fast_second_strip_r(int code, int tile, float alpha) {
  const ResLayout r(code);
  return fast_second_strip_body<kLdCfg3>(r.by, r.bz, r.oJit, r.oRed, kNtCfg3, tile, r.D, alpha, 1, nullptr, nullptr);
}

// The vectors of the solve: soft-abs map, y = (I + E2^T)(I - E1) m', w = y / lam~, x' = (I + E1)(I + E2) w, x = V0 x', P d = V0 (lam0 d'),
// the two row updates; the block sums (log-det, y^T w, sum lam0 d'^2) as wave partials at oS (waves 0 .. 9, stride 4: the caller adds them).
// Waves 0 .. 7 carry the products (mv4: a row's value stays in its four lanes from one stage to the next), waves 8 .. 9 the soft-abs
// map under the second product; five barriers.  Vector block at oVec: e | lam | lam0 -> lam~ | m' | y | x | d' -> lam0 d' | cs, then 16 floats, then oS.
// flags: the kChain* bits.  kChainAssign: x' REPLACES the LDS vector at 4 (resoff & 0xffff).  kChainResident: the updates are
// theta~'[row] += cx x'[row] and p'[row] += cg lam0 d'[row] on the LDS vectors at 4 (resoff & 0xffff) / 4 (resoff >> 16)
// (0: none), the last product and its barrier do not exist.
__device__ __forceinline__ void fast_chain_body(int offV, int offE1, int offE2, int oVec, int D, int DP, int LD, int flags, float alpha,
                                                float* lam_out, float* lamraw_out, float* x_out, float* upd_x, float cx, float* upd_g, float cg, int resoff) {
  HTA_LDS_BASE();
  D = HTA_U(D); DP = HTA_U(DP); LD = HTA_U(LD); flags = HTA_U(flags); oVec = HTA_U(oVec); resoff = HTA_U(resoff);
  const bool skip2 = flags & kChainSkip2, has_x = flags & kChainHasX, resident = flags & kChainResident, sdraw = flags & kChainDraw,
             assign = flags & kChainAssign, strips = flags & kChainStrips;
  const bool mapped = !skip2 && (flags & kChainMapped);                   // lam~, lam0 d' and their block sums are in LDS already (ph_fast_second_strip)
  const float* V = lds + HTA_U(offV); const float* E1 = lds + HTA_U(offE1); const float* E2 = lds + HTA_U(offE2);
  float* vlam = lds + oVec + DP; float* vlt = vlam + DP; float* vm = vlt + DP; float* vy = vm + DP; float* vx = vy + DP; float* vd = vx + DP;
  float* red3 = vd + 2 * DP + MT / 64;
  typedef __attribute__((address_space(1))) float* gf;
  const int tid = threadIdx.x, wave = HTA_U(tid >> 6);
  const int nq = DP >> 2;
  // !skip2: y0 = m' - E1 m' and the partials of E2^T y0 are in LDS already (ph_fast_second): ONE barrier (the soft-abs map) before w.
  // skip2 (no second pass: E2 = 0): y0 is computed here, under the map.
  const int nbar = (skip2 ? 4 : 3) + (resident ? 0 : 1) - (mapped ? 1 : 0);      // barriers of this call
  if (wave >= 10) {                                              // nothing to compute
    for (int k = 0; k < nbar; ++k) __syncthreads();
    return;
  }
  if (wave >= 8) {                                               // soft-abs map (S:120), log-determinant (S:726), d^T P d, lam0 d'
    if (mapped) {                                                // (done by ph_fast_second_strip's idle waves, under its element-wise step)
      for (int k = 0; k < nbar; ++k) __syncthreads();
      return;
    }
    fast_softabs_rows(tid - 512, wave, D, DP, alpha, vlam, vlt, vd, red3, lam_out, lamraw_out, has_x, skip2);
    for (int k = skip2 ? 1 : 0; k < nbar; ++k) __syncthreads();
    return;
  }
  const int row = tid >> 2, c = tid & 3;
  const bool wr = c == 0 && row < D;
  float ux = 0.f, ug = 0.f;                                      // the rows the updates add to: requested now, used at the end
  if (!resident) {
    if (wr && upd_x) ux = ((gf)upd_x)[row];
    if (wr && upd_g) ug = ((gf)upd_g)[row];
  }
  float y = 0.f;
  if (skip2) {                                                   // y0 = m' - E1 m'
    const float e1m = mv4(E1, LD, vm, nq, DP);
    if (row < D) y = vm[row] - e1m;
    if (c == 0 && row < DP) vy[row] = y;
    __syncthreads();                                             // 1: y0
  } else if (row < DP) {                                         // y = y0 + E2^T y0 from the second product's partials (one per macro-tile row)
    const float* p0 = lds + oVec; const float* p1 = lds + oVec + 3 * DP; const float* p2 = lds + oVec + 5 * DP; const float* p3 = lds + oVec + 8 * DP + MT / 64 + 64;
    y = vy[row] + p0[row];
    if (strips) { if (DP > 64) y += p2[row]; }                   // (ph_fast_second_strip: row tiles 0 .. 3 | 4 ..)
    else {
      if (DP > 32) y += p1[row];
      if (DP > 64) y += p2[row];
      if (DP > 96) y += p3[row];
    }
    if (row >= D) y = 0.f;
  }
  if (!mapped) __syncthreads();                                  // lam~, lam0 d' (x may now be overwritten: a row's partial is read by the quad that writes the row)
  float w = 0.f, qd = 0.f;
  if (row < D) { w = sdraw ? y * sqrtf(vlt[row]) : y / vlt[row]; if (c == 0) qd = y * w; }
  if (c == 0 && row < DP) vx[row] = w;
  {
    const float s1 = wave_sum_dpp(qd);
    if ((tid & 63) == 0) { float* r = red3 + 4 * wave; r[0] = 0.f; r[1] = s1; r[2] = 0.f; }
  }
  __syncthreads();                                               // 3: w
  const float* vsrc = vx;
  if (!skip2) {                                                  // w <- w + E2 w
    w += mv4(E2, LD, vx, nq, DP);
    if (c == 0 && row < DP) vy[row] = (row < D) ? w : 0.f;
    vsrc = vy;
  }
  __syncthreads();                                               // 4
  const float xp = w + mv4(E1, LD, vsrc, nq, DP);                // x' = w + E1 w
  if (resident) {
    if (wr && resoff) {
      float* sx = lds + 4 * (resoff & 0xffff); float* sg = lds + 4 * (resoff >> 16);
      if (assign) sx[row] = xp;
      else { sx[row] += cx * xp; sg[row] += cg * vd[row]; }
    }
    return;
  }
  float* vdst = skip2 ? vy : vx;
  if (c == 0 && row < DP) vdst[row] = (row < D) ? xp : 0.f;
  __syncthreads();                                               // 5
  float x, g;
  mv4_dual(V, LD, vdst, vd, nq, DP, x, g);                       // x = V0 x', P d = V0 (lam0 d')
  if (wr) {
    if (x_out) ((gf)x_out)[row] = x;
    if (upd_x) ((gf)upd_x)[row] = ux + cx * x;
    if (upd_g) ((gf)upd_g)[row] = ug + cg * g;
  }
}
__device__ HTA_PH_ATTR void ph_fast_chain(int offV, int offE1, int offE2, int oVec, int D, int DP, int LD, int flags, float alpha,
                                          float* lam_out, float* lamraw_out, float* x_out, float* upd_x, float cx, float* upd_g, float cg, int resoff) {
  fast_chain_body(offV, offE1, offE2, oVec, D, DP, LD, flags, alpha, lam_out, lamraw_out, x_out, upd_x, cx, upd_g, cg, resoff);
}
__device__ HTA_PH_ATTR void ph_fast_chain_r(int code, float alpha, float cx, float cg, int resoff) {      // (ResLayout; the flags above kResFlagShift, RESIDENT among them)
  const ResLayout r(code);
  fast_chain_body(r.bx, r.bz, r.by, r.oJit, r.D, 16 * kNtCfg3, kLdCfg3, (HTA_U(code) >> kResFlagShift) | kChainResident, alpha, nullptr, nullptr, nullptr, nullptr, cx, nullptr, cg, resoff);
}

// The thread index, opaque to the optimiser.  Per-lane global addresses (a.m + b D + i, a.upd_x + b D + row, ...) derived from
// the plain index were computed at the top of the kernel and kept across its 30 out-of-line phase calls - i.e. spilled to
// scratch memory at the 128-register cap of a 1024-thread workgroup (14 stores at the top, 13 reloads scattered over the
// phases, each a round trip beyond the L2: profiles/r02zz WRITE_SIZE 20.7 MB per launch against 0.2 MB of outputs).
// Deriving them from an opaque copy at the point of use keeps them out of the calls' live ranges.
__device__ __forceinline__ int opaque_tid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// the fast solve evaluation of system b (see the block comment above ph_fast_vt); false: nothing written, run the general sequence
// res_xm >= 0: RESIDENT operands - d' at LDS offset 4 (res_xm & 0xffff), m' at 4 (res_xm >> 16) (offsets are multiples of 4: 14 bits each) (eigen-coordinates: no V0 product), the updates
// go to the LDS vectors of res_upd (see ph_fast_chain; 0: none)
// sdraw: the evaluation is the momentum DRAW p = G^(1/2) z - the solve's sequence with m = z (Philox normals of the draw's stream, S:183-184's z)
// and w = y sqrt(lam~); the result goes to a.p_out (resident: it REPLACES the vector of res_upd & 0xffff; res_xm then names theta' and the
// place V0^T z is taken from / put to)
__device__ __forceinline__ bool metric_fast_solve(const MetricArgsT<float>& a, int DP, int LD, int64_t b, int& vres, bool bx3, int tiles,
                                                  int res_xm = -1, int res_upd = 0, bool sdraw = false, bool wb = false) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int D = a.D, tid = threadIdx.x;
  const int nt = DP / 16, k4 = (D + 3) / 4;
  float* const lds0 = reinterpret_cast<float*>(smem_raw);
  const MetricLds lay(DP, LD);
  const int BS = lay.BS, oJit = lay.oJit, oLam = lay.oLam, oLt = lay.oLt, oM = lay.oM, oY = lay.oY, oD = lay.oD, oRed = lay.oRed, oS = lay.oW;
  const int bx = vres >= 0 ? vres : BS;                             // V0: where the previous evaluation left it, else staged into buffer 1
  const int by = bx == 0 ? BS : 0, bz = bx == 2 * BS ? BS : 2 * BS;  // F then E2 | E1
  const uint64_t chain = a.chain_offset + (uint64_t)b;
  __syncthreads();
  if (tid < DP) {
    const int i = opaque_tid();
    const bool in = i < D;
    const float l0 = in ? a.lam0[i] : 0.f;                           // (requested first: the read's latency runs under the jitter's Philox rounds)
    {
      const float ej = (in && a.has_jitter) ? (float)a.jitter * uniform_elem<float>(a.seed, chain, a.draw, PURPOSE_JITTER, a.sub, i) : 0.f;
      lds0[oJit + i] = (wb && bx3 && LD == kLdCfg3) ? sqrtf(ej) : ej;      // (the bfloat16 formation scales BOTH operands: sqrt(e))
    }
    if (res_xm >= 0) {
      lds0[oM + i] = lds0[4 * (res_xm >> 16) + i];
      lds0[oD + i] = lds0[4 * (res_xm & 0xffff) + i];
    } else {
      lds0[oY + 2 * i] = in ? (sdraw ? normal_elem<float>(a.seed, chain, a.draw, 0, i) : a.m[b * D + i]) : 0.f;
      lds0[oY + 2 * i + 1] = (in && a.X) ? a.X[b * D + i] - a.mu[i] : 0.f;
    }
    lds0[oLt + i] = l0;                                              // lam0 (the soft-abs map overwrites it element by element at the end)
    lds0[oLam + i] = 0.f;
  }
  if (vres < 0) ph_stage(a.V0, bx, D, DP, LD);
  vres = bx;
  __syncthreads();
  if (res_xm < 0) ph_fast_vt(bx, oY, oM, oD, DP, LD);
  const bool planes = bx3 && LD == kLdCfg3;                          // F as bfloat16 planes for the bfloat16 form of the second product
  const bool packed = planes && wb && res_xm >= 0;                   // the resident evaluations at kLdCfg3: one packed argument (ResLayout)
  const int rcode = res_code(bx == 0 ? 0 : bx == BS ? 1 : 2, D);  const float e1 = packed ? ph_fast_form_r(rcode, tiles) : (planes && wb) ? ph_fast_form<kLdCfg3, true, true>(bx, by, bz, oJit, oLt, oLam, oRed, tiles, k4, D, LD, nt)
                   : planes ? ph_fast_form<kLdCfg3, true>(bx, by, bz, oJit, oLt, oLam, oRed, tiles, k4, D, LD, nt)
                   : LD == kLdCfg3 ? ph_fast_form<kLdCfg3, false>(bx, by, bz, oJit, oLt, oLam, oRed, tiles, k4, D, LD, nt)
                                   : ph_fast_form<0, false>(bx, by, bz, oJit, oLt, oLam, oRed, tiles, k4, D, LD, nt);
  if (!(e1 <= kSecondE)) return false;
  const bool skip2 = e1 <= kConvE;                                   // (no jitter: F = 0, the shared basis is the answer)
  if (!skip2) {
    float e2;
    // (the bfloat16 form only where the leading dimension is a compile-time constant: the run-time instance needs four registers beyond
    // the caller-saved set, i.e. a save / restore through scratch memory per call that costs more than the product saves)
    if (packed) e2 = ph_fast_second_strip_r(rcode, tiles, (float)a.alpha);
    else if (planes)
      e2 = ph_fast_second_strip<kLdCfg3>(by, bz, oJit, oRed, nt, tiles, D, (float)a.alpha, (res_xm >= 0 || a.X) ? 1 : 0,
                                         (res_xm < 0 && a.lam_out) ? a.lam_out + b * D : nullptr, (res_xm < 0 && a.lamraw_out) ? a.lamraw_out + b * D : nullptr);
    else e2 = LD == kLdCfg3 ? ph_fast_second<kLdCfg3>(by, bz, oJit, oRed, nt, tiles, k4, D, LD)
                            : ph_fast_second<0>(by, bz, oJit, oRed, nt, tiles, k4, D, LD);
    if (!(e2 <= kConvE)) return false;
  }
  if (packed)
    ph_fast_chain_r(rcode | (((skip2 ? kChainSkip2 : 0) | kChainHasX | kChainResident | (sdraw ? kChainDraw | kChainAssign : 0) | kChainStrips | kChainMapped) << kResFlagShift),
                    (float)a.alpha, (float)a.cx, (float)a.cg, res_upd);
  else if (res_xm >= 0)
    ph_fast_chain(bx, bz, by, oJit, D, DP, LD, (skip2 ? kChainSkip2 : 0) | kChainHasX | kChainResident | (sdraw ? kChainDraw | kChainAssign : 0) | (planes ? kChainStrips | kChainMapped : 0),
                  (float)a.alpha, nullptr, nullptr, nullptr, nullptr, (float)a.cx, nullptr,
                  (float)a.cg, res_upd);
  else
    ph_fast_chain(bx, bz, by, oJit, D, DP, LD, (skip2 ? kChainSkip2 : 0) | (a.X ? kChainHasX : 0) | (sdraw ? kChainDraw : 0) | (planes ? kChainStrips | kChainMapped : 0), (float)a.alpha,
                  a.lam_out ? a.lam_out + b * D : nullptr, a.lamraw_out ? a.lamraw_out + b * D : nullptr,
                  sdraw ? a.p_out + b * D : (a.x_out ? a.x_out + b * D : nullptr),
                  a.upd_x ? a.upd_x + b * D : nullptr, (float)a.cx, a.upd_g ? a.upd_g + b * D : nullptr, (float)a.cg, 0);
  if (tid == 0 && (a.logdet_out || a.quad_out || a.logp_out || a.H_out)) {      // (the half steps of a trajectory want none of the scalars)
    const float* r = lds0 + oS;
    float logdet = 0.f, quad = 0.f, dpd = 0.f;
#pragma unroll
    for (int w = 0; w < 10; ++w) { logdet += r[4 * w]; quad += r[4 * w + 1]; dpd += r[4 * w + 2]; }
    const float logp = (a.X || res_xm >= 0) ? (float)a.log_norm - 0.5f * dpd : 0.f;
    if (a.logdet_out) a.logdet_out[b] = logdet;
    if (a.quad_out) a.quad_out[b] = quad;
    if (a.logp_out) a.logp_out[b] = logp;
    if (a.H_out) {
      const float pi_term = (float)D * 1.8378770351409912f;                              // S:712 in float32
      a.H_out[b] = -logp + 0.5f * pi_term + 0.5f * logdet + 0.5f * quad;                 // S:731
    }
  }
  return true;
}

// ---- the trajectory kernel's resident state (round 6) ----------------------------------------------------------------------------
// (ga, gb) = (mu + V0 a', V0 b') for two LDS vectors in eigen-coordinates (mu = nullptr: none): the way back to the caller's coordinates
__device__ HTA_PH_ATTR void ph_res_out(int offV, int offA, int offB, float* ga, float* gb, const float* mu, int D, int DP, int LD) {
  HTA_LDS_BASE();
  D = HTA_U(D); DP = HTA_U(DP); LD = HTA_U(LD);
  typedef __attribute__((address_space(1))) float* gf;
  if (threadIdx.x < 512) {
    float x, g;
    mv4_dual(lds + HTA_U(offV), LD, lds + HTA_U(offA), lds + HTA_U(offB), DP >> 2, DP, x, g);
    const int row = threadIdx.x >> 2;
    if ((threadIdx.x & 3) == 0 && row < D) {
      ((gf)ga)[row] = x + (mu ? ((gcf)mu)[row] : 0.f);
      ((gf)gb)[row] = g;
    }
  }
}
// (a', b') = V0^T (ga - mu, gb): into eigen-coordinates ((m_i, d_i) pairs staged at offMD, then ph_fast_vt)
__device__ __forceinline__ void res_in(int offV, int offMD, int offA, int offB, const float* ga, const float* gb, const float* mu, int D, int DP, int LD) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* const lds0 = reinterpret_cast<float*>(smem_raw);
  __syncthreads();
  if ((int)threadIdx.x < DP) {
    const int i = opaque_tid();
    lds0[offMD + 2 * i] = i < D ? gb[i] : 0.f;
    lds0[offMD + 2 * i + 1] = i < D ? ga[i] - (mu ? mu[i] : 0.f) : 0.f;
  }
  __syncthreads();
  ph_fast_vt(offV, offMD, offB, offA, DP, LD);
}

}  // namespace hta
