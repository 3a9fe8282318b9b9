// rmhmc_fused.hip, device side 3 of 4: the two row-tile layouts of rows4_trajectories (rmhmc_rows4_dev.hpp holds the algorithm) -
// BatchTile, 16 chains per workgroup on v_mfma_f32_16x16x4_f32 (rmhmc_batch_kernel), and Mfma4Tile, four chains per workgroup on
// v_mfma_f32_4x4x1_16b_f32 (rmhmc_mfma4_kernel) - each with the LDS size its launch asks for.
#pragma once
#include "rmhmc_fused_dev.hpp"
#include "rmhmc_rows4_dev.hpp"

namespace hta {

// =============================================================================================
// The same run, 16 chains per workgroup, products on the matrix cores (fp32, D <= 112, pre-drawn momenta, log-det series)
//
// S and P are the same for every chain, so a product pass over 16 chains is S X with X a D x 16 matrix:
// v_mfma_f32_16x16x4_f32 tiles (exact fp32 products, fp32 accumulation; 2048 flop per instruction where the one-chain
// kernel issues one v_fmac_f32_dpp per 128).  Wave w owns the row tile 16w..16w+15: its A fragments (S and P, 28 VGPRs
// each: lane (i, g) holds A[16w+i][28g+j], j < 28 - the K index is permuted so that a lane's share of an operand vector is
// contiguous in LDS) stay in registers for the launch; the B operand of chain column n is X[n][28g+j], seven 16-byte
// LDS reads per vector and pass; the accumulator is C[4g+reg][n]: lane (n, g) OWNS elements 16w+4g .. +3 of chain n's vectors
// and does their element-wise work in registers (four consecutive rows = one Philox block of jitter per evaluation).
// Same streams, same update order, same barriers per pass as rmhmc_fused_kernel; sums run in a different order.
// What it buys is bounded by the fp32 matrix rate (64 flop/clk/SIMD, twice the VALU FMA rate, minus 25 % tile padding at
// D = 100) and by its pass latency (7 row tiles on 4 SIMDs: 2 x 56 MFMAs x 32 clk per first pass): measured against one chain
// per workgroup 0.6x / 0.96x / 1.19x / 1.37x at 512 / 1024 / 2048 / 4096 chains (tools/scratch/pair_check.py), so it is taken
// from 2048 chains per GPU on (hta_set_tuning("rmhmc_batch", 0) off, 2 always); there the per-trajectory Cholesky of the
// momentum draw is the next limit.  TRACK ("rmhmc_pair" = 1, the default): the tracked-products schedule derived in
// rows4_trajectories (4096 chains: 1.56e8 -> 1.84e8 steps/s, 3072: 1.24e8 -> 1.47e8).
// The algorithm is rows4_trajectories (rmhmc_rows4_dev.hpp); BatchTile is this kernel's layout and its products.
// =============================================================================================
constexpr int BNC = 16, BLD = 116, BWV = 7, BNT = 64 * BWV, BSEG = 28, BBUF = 12;

// BKJ: MFMAs per product and row tile = K / 4 (25 for D <= 100, 28 up to 112).  A vector is stored in four segments of BSEG
// floats (16-byte aligned); element `row` sits in segment row / BKJ at offset row % BKJ.
template <int BKJ>
struct BatchTile {
  typedef float T;
  static constexpr int NC = BNC, MSZ = BNC * BLD;
  static constexpr int LDS_FLOATS = BBUF * MSZ + BWV * BNC * 4;       // BBUF vector matrices | red: what a launch asks for (88 KB)
  T *PM, *PMC, *D1, *DC, *D0, *W0, *W1, *EV, *WSA, *WSB, *red;
  int row0, cl, w, g, b_off, own_pos[4];
  bool rok[4], writer;
  T mu_r[4], sd_r[4], Sa[BKJ], Pa[BKJ];

  __device__ __forceinline__ BatchTile(const FusedArgs<float>& a, T* lds) {
    PM = lds; PMC = PM + MSZ; D1 = PMC + MSZ;
    DC = D1 + MSZ;                                        // tracked products: theta_c - mu (D1: theta - mu)
    D0 = DC + MSZ; W0 = D0 + MSZ; W1 = W0 + MSZ; EV = W1 + MSZ;
    // tracked products: 2 pairs x 2 solves x 2 refinement vectors.  The first pair's four ARE the Hamiltonians' D0 W0 W1 EV
    // (contiguous): a Hamiltonian and the first pair of a step are always separated by barriers (block_sums / the solve phases of
    // the second pair), and the whole set stays at 12 matrices = 88 KB
    WSA = D0; WSB = EV + MSZ;
    red = WSB + 4 * MSZ;                                  // [BWV][BNC][4]
    const int tid = threadIdx.x, l = tid & 63;
    w = tid >> 6; cl = l & 15; g = l >> 4;
    const int D = a.D;
    row0 = 16 * w + 4 * g;
    const int arow = 16 * w + cl;
    writer = w == 0 && g == 0;
#pragma unroll
    for (int j = 0; j < BKJ; ++j) {
      const int k = BKJ * g + j;
      const bool ok = arow < D && k < D;
      Sa[j] = ok ? a.S[(int64_t)k * D + arow] : 0.f;      // symmetric: column arow, coalesced over the lanes of a tile
      Pa[j] = ok ? a.P[(int64_t)k * D + arow] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = row0 + e;
      rok[e] = r < D;
      mu_r[e] = rok[e] ? a.mu[r] : 0.f;
      sd_r[e] = rok[e] ? a.S[(int64_t)r * D + r] : 0.f;
    }
    for (int e = tid; e < LDS_FLOATS; e += BNT) lds[e] = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) own_pos[e] = cl * BLD + ((row0 + e) / BKJ) * BSEG + (row0 + e) % BKJ;
    b_off = cl * BLD + BSEG * g;
  }

  __device__ __forceinline__ void put4(T* X, const T (&v)[4]) const {
    if constexpr (BKJ == BSEG) *reinterpret_cast<bf4*>(X + own_pos[0]) = bf4{v[0], v[1], v[2], v[3]};
    else {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (rok[e]) X[own_pos[e]] = v[e];     // rows >= D have no slot in this layout (and stay 0)
    }
  }
  __device__ __forceinline__ void load_b(const T* X, T (&b)[BKJ]) const {
#pragma unroll
    for (int q = 0; q < BKJ / 4; ++q) {
      const bf4 v = *reinterpret_cast<const bf4*>(X + b_off + 4 * q);
      b[4 * q] = v[0]; b[4 * q + 1] = v[1]; b[4 * q + 2] = v[2]; b[4 * q + 3] = v[3];
    }
#pragma unroll
    for (int j = (BKJ / 4) * 4; j < BKJ; ++j) b[j] = X[b_off + j];
  }
  __device__ __forceinline__ void prod2(const T (&A1)[BKJ], const T* X1, const T (&A2)[BKJ], const T* X2, bf4& acc1, bf4& acc2) const {
    T b1[BKJ], b2[BKJ];
    load_b(X1, b1);
    load_b(X2, b2);
#pragma unroll
    for (int j = 0; j < BKJ; ++j) {
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(A1[j], b1[j], acc1, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(A2[j], b2[j], acc2, 0, 0, 0);
    }
  }
  __device__ __forceinline__ void prod1(const T* X, bf4& acc) const {
    T bw[BKJ];
    load_b(X, bw);
    acc = bf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < BKJ; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Sa[j], bw[j], acc, 0, 0, 0);
  }
  __device__ __forceinline__ void prod1_sq(const T* X, bf4& acc) const {
    T be[BKJ];
    load_b(X, be);
#pragma unroll
    for (int j = 0; j < BKJ; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Sa[j] * Sa[j], be[j], acc, 0, 0, 0);
  }
  // two passes of two products (four operand vectors at once do not fit the registers)
  __device__ __forceinline__ void prod4(const T* X1, const T* X2, const T* X3, const T* X4, bf4& p1, bf4& p2, bf4& s3, bf4& s4) const {
    prod2(Pa, X1, Pa, X2, p1, p2);
    prod2(Sa, X3, Sa, X4, s3, s4);
  }
  __device__ __forceinline__ void block_sums(T (&v)[3]) const {
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      v[e] += __shfl_xor(v[e], 16, 64);
      v[e] += __shfl_xor(v[e], 32, 64);
    }
    __syncthreads();
    if (g == 0) {
#pragma unroll
      for (int e = 0; e < 3; ++e) red[(w * BNC + cl) * 4 + e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      T s = 0.f;
#pragma unroll
      for (int i = 0; i < BWV; ++i) s += red[(i * BNC + cl) * 4 + e];
      v[e] = s;
    }
  }
};

template <int BKJ, bool TRACK>
__global__ __launch_bounds__(BNT) void rmhmc_batch_kernel(FusedArgs<float> a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  BatchTile<BKJ> t(a, reinterpret_cast<float*>(smem_raw));
  rows4_trajectories<TRACK>(a, t);
}

// =============================================================================================
// The same run, FOUR chains per workgroup: v_mfma_f32_4x4x1_16b_f32 (16 blocks of 4 x 4, K = 1; fp32, D <= 100)
//
// rmhmc_batch_kernel needs 16 chains per workgroup (the N of its 16 x 16 tile), i.e. C / 16 workgroups: at 1024 chains it
// keeps 64 of the 256 CUs busy.  The 16-block form has N = 4: block b multiplies rows 4b .. 4b+3 of A with the SAME 4
// columns, so one wave covers 64 rows x 4 chains per instruction and two waves a whole product - C / 4 workgroups of two
// waves, one wave per SIMD, the matrix pipes of every CU in use from 512 chains on.  Same flop rate per instruction
// (64 flop / clk / SIMD), same ownership: lane (b, n) = (l >> 2, l & 3) supplies A[64w + l][k] (S and P: 2 x 100 VGPRs for
// the launch) and X[n][k] (LDS, 16-byte reads, the same address for the 16 lanes of a chain) and receives
// C[64w + 4b + r][n], r < 4: four consecutive rows of chain n = one Philox block of jitter, element-wise work in registers.
// Same streams, same update order and barriers as rmhmc_batch_kernel; a product's sum runs over k = 0 .. D-1 in order.
// TRACK ("rmhmc_pair" = 1, the default): the tracked-products schedule derived in rows4_trajectories - 12 products in 5 phases
// per step at K = 2 instead of 16 in 8 (2048 chains: 1.36e8 -> 1.59e8 steps/s, 1536: 1.10e8 -> 1.29e8).  This kernel serves
// 1793 .. 2048 chains per GPU, where two of its workgroups fill a CU's four SIMDs.
// The algorithm is rows4_trajectories (rmhmc_rows4_dev.hpp); Mfma4Tile is this kernel's layout and its products.
// =============================================================================================
constexpr int QNC = 4, QLD = 116, QWV = 2, QNT = 64 * QWV, QK = 100, QBUF = 16;

struct Mfma4Tile {
  typedef float T;
  static constexpr int NC = QNC, MSZ = QNC * QLD;
  static constexpr int LDS_FLOATS = QBUF * MSZ + QWV * QNC * 4;       // QBUF vector matrices | red: what a launch asks for
  T *PM, *PMC, *D0, *D1, *W0, *W1, *EV, *DC, *WSA, *WSB, *red;
  int row0, cl, w, blk, own_off, b_off;
  bool rok[4], writer, rany;
  T mu_r[4], sd_r[4], Sa[QK], Pa[QK];

  __device__ __forceinline__ Mfma4Tile(const FusedArgs<float>& a, T* lds) {
    PM = lds; PMC = PM + MSZ; D0 = PMC + MSZ; D1 = D0 + MSZ; W0 = D1 + MSZ; W1 = W0 + MSZ; EV = W1 + MSZ;
    DC = EV + MSZ;                                        // tracked products: theta_c - mu (D1: theta - mu)
    WSA = DC + MSZ; WSB = WSA + 4 * MSZ;                  // tracked products: 2 pairs x 2 solves x 2 refinement vectors
    red = WSA + 8 * MSZ;                                  // [QWV][QNC][4]
    const int tid = threadIdx.x, l = tid & 63;
    w = tid >> 6; cl = l & 3; blk = l >> 2;
    const int D = a.D;
    row0 = 64 * w + 4 * blk;
    const int arow = 64 * w + l;
    writer = w == 0 && blk == 0;
#pragma unroll
    for (int k = 0; k < QK; ++k) {
      const bool ok = arow < D && k < D;
      Sa[k] = ok ? a.S[(int64_t)k * D + arow] : 0.f;      // symmetric: column arow, coalesced over the lanes
      Pa[k] = ok ? a.P[(int64_t)k * D + arow] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = row0 + e;
      rok[e] = r < D;
      mu_r[e] = rok[e] ? a.mu[r] : 0.f;
      sd_r[e] = rok[e] ? a.S[(int64_t)r * D + r] : 0.f;
    }
    for (int e = tid; e < LDS_FLOATS; e += QNT) lds[e] = 0.f;
    rany = row0 < QLD;                                    // rows 116 .. 127 have no slot (and are >= D)
    own_off = cl * QLD + row0; b_off = cl * QLD;
  }

  __device__ __forceinline__ void put4(T* X, const T (&v)[4]) const { if (rany) *reinterpret_cast<bf4*>(X + own_off) = bf4{v[0], v[1], v[2], v[3]}; }
  // One wave per SIMD: nothing else hides an LDS round trip, so the operand chunks (4 values of k per 16-byte read) are
  // fetched two chunks (16 MFMAs = 128 clocks) ahead of their use.
  __device__ __forceinline__ bf4 chunk(const T* X, int q) const { return *reinterpret_cast<const bf4*>(X + b_off + 4 * q); }
  // two products with one pass over k: acc1 = A1 X1, acc2 = A2 X2 (two independent accumulator chains)
  __device__ __forceinline__ void prod2(const T (&A1)[QK], const T* X1, const T (&A2)[QK], const T* X2, bf4& acc1, bf4& acc2) const {
    bf4 c1 = chunk(X1, 0), c2 = chunk(X2, 0), n1 = chunk(X1, 1), n2 = chunk(X2, 1);
#pragma unroll
    for (int q = 0; q < QK / 4; ++q) {
      bf4 f1 = n1, f2 = n2;
      if (q + 2 < QK / 4) { f1 = chunk(X1, q + 2); f2 = chunk(X2, q + 2); }
      __builtin_amdgcn_sched_barrier(0);                    // (the scheduler otherwise sinks the reads next to their use)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(A1[4 * q + u], c1[u], acc1, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_4x4x1f32(A2[4 * q + u], c2[u], acc2, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      c1 = n1; c2 = n2; n1 = f1; n2 = f2;
    }
  }
  __device__ __forceinline__ void prod1(const T* X, bf4& acc) const {
    bf4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};      // even / odd k: two chains keep the pipe issuing
    bf4 c = chunk(X, 0), n1 = chunk(X, 1), n2 = chunk(X, 2);
#pragma unroll
    for (int q = 0; q < QK / 4; ++q) {
      bf4 f = n2;
      if (q + 3 < QK / 4) f = chunk(X, q + 3);
      __builtin_amdgcn_sched_barrier(0);
      sa = __builtin_amdgcn_mfma_f32_4x4x1f32(Sa[4 * q], c[0], sa, 0, 0, 0);
      sb = __builtin_amdgcn_mfma_f32_4x4x1f32(Sa[4 * q + 1], c[1], sb, 0, 0, 0);
      sa = __builtin_amdgcn_mfma_f32_4x4x1f32(Sa[4 * q + 2], c[2], sa, 0, 0, 0);
      sb = __builtin_amdgcn_mfma_f32_4x4x1f32(Sa[4 * q + 3], c[3], sb, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      c = n1; n1 = n2; n2 = f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = sa[e] + sb[e];
  }
  __device__ __forceinline__ void prod1_sq(const T* X, bf4& acc) const {
    bf4 c = chunk(X, 0), n1 = chunk(X, 1), n2 = chunk(X, 2), s2b = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < QK / 4; ++q) {
      bf4 f = n2;
      if (q + 3 < QK / 4) f = chunk(X, q + 3);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 4; u += 2) {
        acc = __builtin_amdgcn_mfma_f32_4x4x1f32(Sa[4 * q + u] * Sa[4 * q + u], c[u], acc, 0, 0, 0);
        s2b = __builtin_amdgcn_mfma_f32_4x4x1f32(Sa[4 * q + u + 1] * Sa[4 * q + u + 1], c[u + 1], s2b, 0, 0, 0);
      }
      c = n1; n1 = n2; n2 = f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += s2b[e];
  }
  __device__ __forceinline__ void prod4(const T* X1, const T* X2, const T* X3, const T* X4, bf4& p1, bf4& p2, bf4& s3, bf4& s4) const {
    bf4 c1 = chunk(X1, 0), c2 = chunk(X2, 0), c3 = chunk(X3, 0), c4 = chunk(X4, 0);
#pragma unroll
    for (int q = 0; q < QK / 4; ++q) {
      bf4 n1 = c1, n2 = c2, n3 = c3, n4 = c4;
      if (q + 1 < QK / 4) { n1 = chunk(X1, q + 1); n2 = chunk(X2, q + 1); n3 = chunk(X3, q + 1); n4 = chunk(X4, q + 1); }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        p1 = __builtin_amdgcn_mfma_f32_4x4x1f32(Pa[4 * q + u], c1[u], p1, 0, 0, 0);
        p2 = __builtin_amdgcn_mfma_f32_4x4x1f32(Pa[4 * q + u], c2[u], p2, 0, 0, 0);
        s3 = __builtin_amdgcn_mfma_f32_4x4x1f32(Sa[4 * q + u], c3[u], s3, 0, 0, 0);
        s4 = __builtin_amdgcn_mfma_f32_4x4x1f32(Sa[4 * q + u], c4[u], s4, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      c1 = n1; c2 = n2; c3 = n3; c4 = n4;
    }
  }
  __device__ __forceinline__ void block_sums(T (&v)[3]) const {
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      v[e] += __shfl_xor(v[e], 4, 64);
      v[e] += __shfl_xor(v[e], 8, 64);
      v[e] += __shfl_xor(v[e], 16, 64);
      v[e] += __shfl_xor(v[e], 32, 64);
    }
    __syncthreads();
    if (blk == 0) {
#pragma unroll
      for (int e = 0; e < 3; ++e) red[(w * QNC + cl) * 4 + e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      T s = 0.f;
#pragma unroll
      for (int i = 0; i < QWV; ++i) s += red[(i * QNC + cl) * 4 + e];
      v[e] = s;
    }
  }
};

template <bool TRACK>
__global__ __launch_bounds__(QNT) void rmhmc_mfma4_kernel(FusedArgs<float> a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  Mfma4Tile t(a, reinterpret_cast<float*>(smem_raw));
  rows4_trajectories<TRACK>(a, t);
}

}  // namespace hta
