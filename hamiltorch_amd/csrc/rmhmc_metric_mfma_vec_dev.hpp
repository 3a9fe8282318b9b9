// Matrix-core metric kernel: cross-lane reductions on DPP, the matrix-vector products with 8 lanes per row, staging of dense matrices
// into LDS, and the panel Cholesky.
#pragma once
#include "rmhmc_metric_mfma_gemm_dev.hpp"

namespace hta {

// Cross-lane sums / maxima as DPP operands of the adding instruction (quad permutes, row_half_mirror, row_mirror; the four rows
// of a wave through v_readlane): __shfl_xor compiles to ds_bpermute_b32 - an LDS round trip per butterfly step, six in a row for
// a wave sum (~700 cycles; a block reduction in this file cost ~1.9 k, measured).  Every lane gets the result.
template <int CTRL> __device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float lane_f(float v, int lane) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane)); }
__device__ __forceinline__ float sum8_dpp(float v) {            // aligned groups of 8 lanes
  v += dpp_f<0xB1>(v);                                          // quad_perm [1,0,3,2]
  v += dpp_f<0x4E>(v);                                          // quad_perm [2,3,0,1]
  v += dpp_f<0x141>(v);                                         // row_half_mirror: the other quad of the 8
  return v;
}
__device__ __forceinline__ float sum16_dpp(float v) { v = sum8_dpp(v); v += dpp_f<0x140>(v); return v; }      // row_mirror: the other half of the 16
__device__ __forceinline__ float max16_dpp(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v)); v = fmaxf(v, dpp_f<0x4E>(v)); v = fmaxf(v, dpp_f<0x141>(v)); v = fmaxf(v, dpp_f<0x140>(v));
  return v;
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v = sum16_dpp(v);
  return (lane_f(v, 0) + lane_f(v, 16)) + (lane_f(v, 32) + lane_f(v, 48));
}
__device__ __forceinline__ float wave_max_dpp(float v) {
  v = max16_dpp(v);
  return fmaxf(fmaxf(lane_f(v, 0), lane_f(v, 16)), fmaxf(lane_f(v, 32), lane_f(v, 48)));
}
static_assert(MT / 64 == 16, "the block reductions below fold the 16 wave results in one DPP row");
__device__ __forceinline__ float block_sum_dpp(float v, float* red) {
  v = wave_sum_dpp(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return sum16_dpp(red[threadIdx.x & 15]);
}
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max_dpp(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return max16_dpp(red[threadIdx.x & 15]);
}

// Maxima of NON-NEGATIVE values (|x|, or 0) as unsigned maxima of their bit patterns: the DPP operand folds into v_max_u32 - one instruction per
// butterfly step where fmaxf takes three (a v_mov_dpp and a canonicalising v_max of each operand); a NaN orders above every number and survives.
template <int CTRL> __device__ __forceinline__ unsigned dpp_u(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true); }
__device__ __forceinline__ unsigned max16_u(unsigned v) {
  v = max(v, dpp_u<0xB1>(v)); v = max(v, dpp_u<0x4E>(v)); v = max(v, dpp_u<0x141>(v)); v = max(v, dpp_u<0x140>(v));
  return v;
}
__device__ __forceinline__ float wave_max_nn(float x) {
  const unsigned v = max16_u(__float_as_uint(x));
  return __uint_as_float(max(max((unsigned)__builtin_amdgcn_readlane((int)v, 0), (unsigned)__builtin_amdgcn_readlane((int)v, 16)),
                             max((unsigned)__builtin_amdgcn_readlane((int)v, 32), (unsigned)__builtin_amdgcn_readlane((int)v, 48))));
}
// max |v_i| over a vector of n <= 128 LDS floats whose padding entries are zero (no predicate: the index is clamped)
__device__ __forceinline__ float wave_max_abs(const float* v, int n) {
  const int lane = threadIdx.x & 63;
  const unsigned a = __float_as_uint(v[min(lane, n - 1)]) & 0x7fffffffu, b = __float_as_uint(v[min(lane + 64, n - 1)]) & 0x7fffffffu;
  return wave_max_nn(__uint_as_float(max(a, b)));
}
// a block maximum (non-negative values) with ONE barrier, for call sites whose previous use of `red` is already fenced by a barrier every wave has passed
__device__ __forceinline__ float block_max1(float v, float* red) {
  v = wave_max_nn(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return __uint_as_float(max16_u(__float_as_uint(red[threadIdx.x & 15])));
}

// out[row] = sum_k M(row, k) v[k] with 8 lanes per row (rows 0 .. 127 of the workgroup's 1024 threads); M(row, k) =
// TRANS ? M[k * ld + row] : M[row * ld + k]; n = vector length (rows and columns).  Every lane of a row's group returns the sum.
// Row-wise (TRANS = false) the 8 lanes of a row read it as 16-byte quads - quad seg + 8 u of the row and of v, zero padded to a
// multiple of 4 - : 8 LDS instructions per lane instead of 28 (the 4-byte form is bound by the LDS instruction rate: 448
// wave-reads of 2+ clocks for a 40 KB matrix - 3 k cycles per product, measured; the quads: ~1 k).  Column-wise (TRANS) keeps
// 4-byte reads of 8 consecutive rows per k.
template <bool TRANS> __device__ __forceinline__ float mv8(const float* M, int ld, const float* v, int n) {
  const int row = threadIdx.x >> 3, seg = threadIdx.x & 7;
  float acc0 = 0.f, acc1 = 0.f;
  if (!TRANS) {
    if (row < n) {
      const int nq = (n + 3) >> 2;
      const float* mr = M + row * ld;
      f4 mq[4], vq[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = seg + 8 * u;
        const bool on = q < nq;
        mq[u] = on ? *reinterpret_cast<const f4*>(mr + 4 * q) : f4{0.f, 0.f, 0.f, 0.f};
        vq[u] = on ? *reinterpret_cast<const f4*>(v + 4 * q) : f4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc0 = fmaf(mq[u][0], vq[u][0], acc0); acc1 = fmaf(mq[u][1], vq[u][1], acc1);
        acc0 = fmaf(mq[u][2], vq[u][2], acc0); acc1 = fmaf(mq[u][3], vq[u][3], acc1);
      }
    }
  } else if (row < n) {
    // n <= 112: 14 steps of 8, seven operand pairs in flight at a time
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float mv[7], vv[7];
#pragma unroll
      for (int u = 0; u < 7; ++u) {
        const int k = seg + 8 * (7 * h + u);
        const bool on = k < n;
        mv[u] = on ? (TRANS ? M[k * ld + row] : M[row * ld + k]) : 0.f;
        vv[u] = on ? v[k] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 7; ++u) { if (u & 1) acc1 = fmaf(mv[u], vv[u], acc1); else acc0 = fmaf(mv[u], vv[u], acc0); }
    }
  }
  float acc = acc0 + acc1;
  return sum8_dpp(acc);
}

// y = M v for a SYMMETRIC dense row-major [n][n] matrix in global memory (P; L2 resident): thread (column c = tid & 127,
// slice q = tid >> 7) sums M[k][c] v[k] over k = q, q + 8, ... - consecutive lanes read consecutive addresses, all 14 loads
// of a thread are in flight together, no cross-lane reduction.  The 8 slice partials meet in `part` ([8][128] floats of
// LDS); after the barrier inside, y[c] = sum_q part[q][c] is returned to the threads tid < 128 (0 elsewhere).
__device__ __forceinline__ float gmv_sym(const __attribute__((address_space(1))) float* M, const float* v, int n, float* part) {
  const int c = threadIdx.x & 127, q = threadIdx.x >> 7;
  float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float mv[7];
#pragma unroll
    for (int u = 0; u < 7; ++u) {
      const int k = q + 8 * (7 * h + u);
      mv[u] = (c < n && k < n) ? M[k * n + c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 7; ++u) {
      const int k = q + 8 * (7 * h + u);
      const float vk = k < n ? v[k] : 0.f;
      if (u & 1) acc1 = fmaf(mv[u], vk, acc1); else acc0 = fmaf(mv[u], vk, acc0);
    }
  }
  part[q * 128 + c] = acc0 + acc1;
  __syncthreads();
  float y = 0.f;
  if (threadIdx.x < 128) {
#pragma unroll
    for (int t = 0; t < 8; ++t) y += part[t * 128 + threadIdx.x];
  }
  return y;
}

// the same for a lower-triangular M: out[row] = sum_{k <= row} M[row][k] v[k]  (p = L z)
__device__ __forceinline__ float mv8_lower(const float* M, int ld, const float* v, int n) {
  const int row = threadIdx.x >> 3, seg = threadIdx.x & 7;
  float acc = 0.f;
  if (row < n)
    for (int k = seg; k <= row; k += 8) acc = fmaf(M[row * ld + k], v[k], acc);
  return sum8_dpp(acc);
}

// a zero-padded [DP][LD] copy of a dense row-major [D][D] matrix in global memory
__device__ __forceinline__ void stage_dense(const __attribute__((address_space(1))) float* src, float* dst, int D, int DP, int LD) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int h = 0; h < 2; ++h) {                              // DP <= 112, LD <= 116: seven loads of a thread in flight at a time
    float v[7];
    const int j = lane + 64 * h;
#pragma unroll
    for (int t = 0; t < 7; ++t) { const int i = wave + 16 * t; v[t] = (i < D && j < D) ? src[i * D + j] : 0.f; }
#pragma unroll
    for (int t = 0; t < 7; ++t) { const int i = wave + 16 * t; if (i < DP && j < LD) dst[i * LD + j] = v[t]; }
  }
}

// Right-looking Cholesky of the symmetric [D][D] matrix in G (leading dimension LD, zero padded to DP) in panels of 16
// columns: the 16 x 16 diagonal block is factored and inverted by one wave (lane = row of the block; a column step is a
// broadcast of the pivot row through LDS), the panel below it is L21 = A21 inv(L11)^T and the trailing matrix loses
// L21 L21^T, both as MFMA tiles (K = 16: four instructions per tile).  The factor replaces the lower triangle; W is a
// [16][20] scratch block.  A non-positive pivot yields NaN, as the reference's cholesky raises.
__device__ __forceinline__ float lane_bcast(float x, int lane) {       // v_readlane_b32: `lane` is uniform (a compile-time constant here)
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane));
}

__device__ HTA_PH_ATTR void mfma_cholesky(int offG, int D, int DP, int LD, int offW) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* const G = reinterpret_cast<float*>(smem_raw) + __builtin_amdgcn_readfirstlane(offG);
  float* const W = reinterpret_cast<float*>(smem_raw) + __builtin_amdgcn_readfirstlane(offW);
  D = __builtin_amdgcn_readfirstlane(D); DP = __builtin_amdgcn_readfirstlane(DP); LD = __builtin_amdgcn_readfirstlane(LD);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int nt = DP / 16;
  for (int pb = 0; pb < nt; ++pb) {
    const int c0 = 16 * pb;
    __syncthreads();
    if (wave == 0) {
      // --- unblocked factorisation of the diagonal block, lane i (< 16) owns row i; columns past D are the identity
      float row[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) row[j] = (lane < 16) ? G[(c0 + lane) * LD + c0 + j] : 0.f;
      const bool live = lane < 16 && c0 + lane < D;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const bool cj = c0 + j < D;
        float d = lane_bcast(row[j], j);                       // pivot
        d = cj ? sqrtf(d) : 1.f;
        const float inv = 1.f / d;
        float lij = (lane == j) ? d : row[j] * inv;            // column j of L (rows >= j)
        if (!cj) lij = (lane == j) ? 1.f : 0.f;
        if (lane < j) lij = 0.f;
        row[j] = lij;
#pragma unroll
        for (int k = j + 1; k < 16; ++k) {
          const float lkj = lane_bcast(lij, k);                // L[k][j]
          if (lane >= k) row[k] -= lij * lkj;
        }
      }
      if (live) {
#pragma unroll
        for (int j = 0; j < 16; ++j) G[(c0 + lane) * LD + c0 + j] = (j <= lane) ? row[j] : 0.f;
      }
      // --- inverse of the triangular block, row by row: inv(L)[i][:] = (e_i - sum_{k<i} L[i][k] inv(L)[k][:]) / L[i][i];
      //     lane = column of the inverse
      float invc[16];                                          // invc[i] = inv(L)[i][lane]
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float acc = (lane == i) ? 1.f : 0.f;
#pragma unroll
        for (int k = 0; k < i; ++k) acc -= lane_bcast(row[k], i) * invc[k];
        invc[i] = acc / lane_bcast(row[i], i);
      }
      if (lane < 16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) W[i * 20 + lane] = invc[i];   // W[i][c] = inv(L11)[i][c]
      }
    }
    __syncthreads();
    // --- panel: L21 = A21 inv(L11)^T, i.e. L21[m][n] = sum_k A21[m][k] inv(L11)[n][k]; one wave per 16-row tile
    const int below = nt - pb - 1;
    for (int t = wave; t < below; t += MT / 64) {
      const int r0 = 16 * (pb + 1 + t);
      f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(G[(r0 + li) * LD + c0 + 4 * kk + lk], W[li * 20 + 4 * kk + lk], acc, 0, 0, 0);
      // all of the tile's operands are in registers before any lane stores (the MFMA consumed them)
#pragma unroll
      for (int r = 0; r < 4; ++r) G[(r0 + 4 * lk + r) * LD + c0 + li] = acc[r];
    }
    __syncthreads();
    // --- trailing update: A22 -= L21 L21^T on the lower tiles (I >= J)
    const int ntr = below * (below + 1) / 2;
    for (int t = wave; t < ntr; t += MT / 64) {
      int J, I;
      upper_tile(t, below, J, I);                              // J <= I
      const int r0 = 16 * (pb + 1 + I), q0 = 16 * (pb + 1 + J);
      f4 acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = G[(r0 + 4 * lk + r) * LD + q0 + li];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(-G[(r0 + li) * LD + c0 + 4 * kk + lk], G[(q0 + li) * LD + c0 + 4 * kk + lk], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) G[(r0 + 4 * lk + r) * LD + q0 + li] = acc[r];
    }
  }
  __syncthreads();
}

}  // namespace hta
