// rmhmc_fused.hip, device side 1 of 4: the panel Cholesky in LDS that the one-chain kernel (rmhmc_fused_chain_dev.hpp) and the
// workgroup momentum draw (rmhmc_fused_momentum_dev.hpp) factor with, and the constants those two headers share.
#pragma once
#include "common.hpp"

namespace hta {

constexpr int FNT = 256;          // 4 waves: (row block of 64) x (half of the contraction range)
constexpr int FCB = 4;            // Cholesky panel width

// The register split of a SIMD between the two kernels that run side by side under the momentum / trajectory overlap:
// rmhmc_fused_kernel_wide takes kFusedWideVgprs, rmhmc_momentum_wave_kernel is capped at 512 - kFusedWideVgprs, so that one
// workgroup's wave of the former and the waves of the latter use a SIMD's 512 registers exactly.
constexpr int kFusedWideVgprs = 288;

template <typename T> __device__ __forceinline__ T fast_rsqrt(T v) { return (T)1 / sqrt(v); }
template <> __device__ __forceinline__ float fast_rsqrt<float>(float v) { return __builtin_amdgcn_rsqf(v); }   // v_rsq_f32, 1 ulp

// W = P + diag(ev) -> its Cholesky factor (strictly-lower part in W, diagonal in dg), right-looking in panels of
// FCB columns: the panel rows are one thread each (the FCB x FCB diagonal block is refactored by every thread from
// LDS: no extra barrier), the rank-FCB trailing update a 16 x 16 thread tile with the panel rows it needs in
// registers.  Returns this thread's share of log |F| (sum over threads = log |F|).
template <typename T>
__device__ __forceinline__ T chol_in_lds(const T* __restrict__ P, const T* ev, T* W, T* dg, int D, int ld, int tid) {
  __syncthreads();
  {
    const float invD = 1.0f / (float)D;
    for (int e0 = tid; e0 < D * D; e0 += 8 * FNT) {       // 8 independent L2 loads in flight per thread
      T t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { const int e = e0 + u * FNT; t[u] = e < D * D ? P[e] : (T)0; }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + u * FNT;
        int i = (int)(((float)e + 0.5f) * invD);             // e / D without the integer divide (e < 2^14)
        const int j = e - i * D;
        if (e < D * D && j <= i) W[i * ld + j] = t[u] + (i == j ? ev[i] : (T)0);
      }
    }
  }
  __syncthreads();
  const int tx = tid & 15, ty = tid >> 4;
  for (int kb = 0; kb < D; kb += FCB) {
    const int nb = min(FCB, D - kb);
    // --- panel: diagonal block factor (registers, every thread), then this thread's row of the panel
    T Ld[FCB][FCB], rinv[FCB];
#pragma unroll
    for (int c = 0; c < FCB; ++c)
#pragma unroll
      for (int c2 = 0; c2 < FCB; ++c2) Ld[c][c2] = (c < nb && c2 <= c) ? W[(kb + c) * ld + kb + c2] : (T)(c == c2);
#pragma unroll
    for (int c = 0; c < FCB; ++c) {
#pragma unroll
      for (int c2 = 0; c2 < c; ++c2) {
        T v = Ld[c][c2];
#pragma unroll
        for (int c3 = 0; c3 < c2; ++c3) v = fma(-Ld[c][c3], Ld[c2][c3], v);
        Ld[c][c2] = v * rinv[c2];
      }
      T v = Ld[c][c];
#pragma unroll
      for (int c3 = 0; c3 < c; ++c3) v = fma(-Ld[c][c3], Ld[c][c3], v);
      rinv[c] = fast_rsqrt<T>(v);
      Ld[c][c] = v * rinv[c];
    }
    T lrow[FCB];
    const int i = kb + FCB + tid;                       // rows below the diagonal block: one thread each
    const bool below = i < D;
    if (below) {
#pragma unroll
      for (int c = 0; c < FCB; ++c) {
        T v = c < nb ? W[i * ld + kb + c] : (T)0;
#pragma unroll
        for (int c3 = 0; c3 < c; ++c3) v = fma(-lrow[c3], Ld[c][c3], v);
        lrow[c] = v * rinv[c];
      }
    }
    __syncthreads();                                     // every thread has read the old panel / diagonal block
    if (below) {
#pragma unroll
      for (int c = 0; c < FCB; ++c) if (c < nb) W[i * ld + kb + c] = lrow[c];
    }
#pragma unroll
    for (int c = 0; c < FCB; ++c) {                      // rows of the diagonal block itself (static indices: Ld stays in registers)
      if (tid == c && c < nb) {
        dg[kb + c] = Ld[c][c];
#pragma unroll
        for (int c2 = 0; c2 < c; ++c2) W[(kb + c) * ld + kb + c2] = Ld[c][c2];
      }
    }
    __syncthreads();
    // --- trailing update with the finished panel: rows ii = r0 + 16 a (a-th slot of ty), columns j = c0 + 16 b (tx)
    const int rbase = kb + FCB + ty, cbase = kb + FCB + tx;
    for (int ii = rbase; ii < D; ii += 16) {
      T* wrow = W + ii * ld;
      T li[FCB];
#pragma unroll
      for (int c = 0; c < FCB; ++c) li[c] = wrow[kb + c];
      for (int j = cbase; j <= ii; j += 32) {            // two column slots per trip: both sets of loads in flight together
        const int j2 = j + 16;
        const bool two = j2 <= ii;
        const T* p1 = W + j * ld + kb;
        const T* p2 = W + (two ? j2 : j) * ld + kb;
        T l1[FCB], l2[FCB];
#pragma unroll
        for (int c = 0; c < FCB; ++c) { l1[c] = p1[c]; l2[c] = p2[c]; }
        T v1 = wrow[j], v2 = wrow[two ? j2 : j];
#pragma unroll
        for (int c = 0; c < FCB; ++c) { v1 = fma(-li[c], l1[c], v1); v2 = fma(-li[c], l2[c], v2); }
        wrow[j] = v1;
        if (two) wrow[j2] = v2;
      }
    }
    __syncthreads();
  }
  return tid < D ? (T)2 * log(dg[tid]) : (T)0;
}

}  // namespace hta
