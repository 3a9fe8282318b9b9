// rmhmc_fused.hip, device side 4 of 4: the momentum draws of a block of trajectories ahead of the trajectory kernels - a
// factorisation per draw on a workgroup (rmhmc_momentum_kernel) or on one wave (rmhmc_momentum_wave_kernel), or no factorisation
// per draw at all (rmhmc_momentum_split_kernel) - and inverse_from_eigen_kernel, which builds the shared S = P^-1 once per run.
#pragma once
#include "philox.hpp"
#include "rmhmc_fused_chol_dev.hpp"

namespace hta {

// The momentum draws of a block of trajectories, off the chains' critical path: task (t, c) -> p = chol(P + diag(e)) z
// with the jitter sub-stream 0 and the normals of (chain c, trajectory traj_offset + t)  (S:183-184).  One workgroup per
// task at a time, 3 per CU: the factorisations of different tasks overlap each other's LDS latency, which the chain-
// serial kernel cannot do.  Without jitter the factor is the same for every task and is computed once per workgroup.
// LDS in elements of T: W[D][ld] | dg[128] | ev[128] | z[128] - what the kernel carves below and the launcher asks for
__host__ __device__ constexpr size_t momentum_lds_elems(int D, int ld) { return (size_t)D * ld + 3 * 128; }
template <typename T>
__global__ __launch_bounds__(FNT) void rmhmc_momentum_kernel(const T* __restrict__ P, int has_jitter, T jitter, int64_t C, int D,
                                                             int ld, int n_traj, int traj_offset, uint64_t seed,
                                                             uint64_t chain_offset, T* __restrict__ p_ws) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* W = reinterpret_cast<T*>(smem_raw);
  T* dg = W + D * ld; T* ev = dg + 128; T* z = ev + 128;
  const int tid = threadIdx.x;
  const int64_t ntask = (int64_t)n_traj * C;
  bool have = false;
  for (int64_t task = blockIdx.x; task < ntask; task += gridDim.x) {
    const int t = (int)(task / C);
    const int64_t c = task - (int64_t)t * C;
    const uint64_t chain = chain_offset + (uint64_t)c;
    const uint32_t n = (uint32_t)(traj_offset + t);
    __syncthreads();
    if (tid < D) {
      ev[tid] = has_jitter ? jitter * uniform_elem<T>(seed, chain, n, PURPOSE_JITTER, 0, tid) : (T)0;
      z[tid] = normal_elem<T>(seed, chain, n, 0, tid);
    }
    if (has_jitter || !have) { chol_in_lds<T>(P, ev, W, dg, D, ld, tid); have = true; }
    __syncthreads();
    if (tid < D) {                                        // row tid of p = L z: the twin of fused_body's in-kernel draw (one helper for both moves the code object)
      T acc0 = dg[tid] * z[tid], acc1 = 0;
      const T* rowp = W + tid * ld;
      int k = 0;
      for (; k + 1 < tid; k += 2) { acc0 = fma(rowp[k], z[k], acc0); acc1 = fma(rowp[k + 1], z[k + 1], acc1); }
      if (k < tid) acc0 = fma(rowp[k], z[k], acc0);
      p_ws[task * D + tid] = acc0 + acc1;
    }
  }
}

// The same draws WITHOUT a factorisation per draw (round 3; tuning key "rmhmc_momsplit", default 1).  On the fused route the
// metric of an evaluation is G = P + diag(e), e = jitter * u (S:113-121 with the soft-abs map the identity), and S:183-184
// asks for p ~ N(0, G).  With L_P = chol(P) - ONE factor per target, computed by the setup on the host in double - and two
// independent standard-normal vectors,
//     p = L_P z1 + sqrt(e) . z2      has covariance  L_P L_P^T + diag(e) = G  exactly,
// the distribution MultivariateNormal(0, G).sample() draws from, given the same u; what changes is the map from the
// uniform / normal draws to p (the reference's, and "rmhmc_momsplit" = 0: chol(G) z), i.e. the realisation, not the law -
// like every other draw of this engine against torch's generator.  z1 is the momentum stream the factorising kernels use
// (normal sub-stream 0), u their jitter stream (sub-stream 0), z2 normal sub-stream 1; oracle/hmc_oracle.py::rm_gibbs_split
// is the same map.  Cost per draw: a D x D triangular matrix-vector product and three Philox passes instead of D^3 / 3
// flops of latency-bound panels: 1.9 ms -> 0.1 ms per 100 trajectories at 1024 chains.
// One wave per task; L_P transposed and zero-filled above the diagonal in LDS ([k][i]: the lanes of a wave read consecutive
// rows i, and the k loop has ONE trip count for every lane - the terms beyond the diagonal add an exact zero, so the sums
// are the ascending-k single-accumulator sums of the oracle); a lane carries its rows i = l and l + 64 through the same loop
// (two accumulators, z1 read as 16-byte broadcasts).  The three Philox streams of a draw go to three groups of lanes (z1:
// lanes 0 .., z2: lanes 32 .., u: lanes 0 .. again behind z1 when D > 128 never happens: D <= 128 means <= 32 blocks per
// stream), so a wave's critical path holds one normal4 and one uniform pass instead of three Philox passes and two normal4.
// Staging walks rows (no integer division).  First version: 0.33 ms per 102 400 draws at D = 100 (rocprofv3, profiles/r03p_*).
// LDS in elements of T: Lt[D + 4][D | 1] (+ 128), rounded up to 16 bytes | per wave z1[128] sqrt(e)[128] z2[128], four waves
constexpr int kSplitWaveElems = 3 * 128;
__host__ __device__ constexpr int momentum_split_lt_elems(int D) { return ((D + 4) * (D | 1) + 128 + 3) & ~3; }
__host__ __device__ constexpr size_t momentum_split_lds_elems(int D) { return (size_t)momentum_split_lt_elems(D) + 4 * kSplitWaveElems; }
template <typename T>
__global__ __launch_bounds__(256) void rmhmc_momentum_split_kernel(const T* __restrict__ LP, T jitter, int64_t C, int D, int n_traj,
                                                                   int traj_offset, uint64_t seed, uint64_t chain_offset,
                                                                   T* __restrict__ p_ws) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* Lt = reinterpret_cast<T*>(smem_raw);                 // [D + 4][ldt] (+ 128): Lt[k * ldt + i] = L_P[i][k]; 0 for k > i and in the rows k >= D
  const int ldt = D | 1;
  const int lt_elems = momentum_split_lt_elems(D);
  T* zb = Lt + lt_elems;                                  // per wave: z1[128] | sqrt(e) [128] | z2[128], 16-byte aligned
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  T* z1 = zb + w * kSplitWaveElems; T* se = z1 + 128; T* z2 = se + 128;
  for (int i = w; i < D; i += 4)
    for (int k = l; k < D; k += 64) Lt[k * ldt + i] = (k <= i) ? LP[(size_t)i * D + k] : (T)0;
  for (int e = D * ldt + tid; e < lt_elems; e += 256) Lt[e] = (T)0;
  for (int e = l; e < 128; e += 64) z1[e] = (T)0;         // the k loop runs to a multiple of 4
  __syncthreads();
  const int64_t ntask = (int64_t)n_traj * C;
  const int nblk = (D + 3) / 4;                           // <= 32
  const int D4 = (D + 3) & ~3;
  const bool row2 = l + 64 < D;
  const T* Lc = Lt + l;
  for (int64_t task = (int64_t)blockIdx.x * 4 + w; task < ntask; task += (int64_t)gridDim.x * 4) {
    const int t = (int)(task / C);
    const int64_t c = task - (int64_t)t * C;
    const uint64_t chain = chain_offset + (uint64_t)c;
    const uint32_t n = (uint32_t)(traj_offset + t);
    // element j of a stream = Philox block j / 4, slot j % 4 (philox.hpp)
    const int b = l & 31;
    if (b < nblk) {
      T a[4];
      if (l < 32) {
        normal4<T>(philox_block(seed, chain, n, PURPOSE_MOMENTUM, 0, (uint32_t)b), a);
#pragma unroll
        for (int q = 0; q < 4; ++q) z1[4 * b + q] = (4 * b + q < D) ? a[q] : (T)0;
        const U4 r = philox_block(seed, chain, n, PURPOSE_JITTER, 0, (uint32_t)b);
        const T u[4] = {u23<T>(r.x), u23<T>(r.y), u23<T>(r.z), u23<T>(r.w)};
#pragma unroll
        for (int q = 0; q < 4; ++q) se[4 * b + q] = sqrt(jitter * u[q]);
      } else {
        normal4<T>(philox_block(seed, chain, n, PURPOSE_MOMENTUM, 1, (uint32_t)b), a);
#pragma unroll
        for (int q = 0; q < 4; ++q) z2[4 * b + q] = a[q];
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    T acc0 = 0, acc1 = 0;
#pragma unroll 2
    for (int k = 0; k < D4; k += 4) {                     // ascending k, one accumulator per row: the oracle's order
      T zz[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) zz[q] = z1[k + q];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc0 = fma(Lc[(k + q) * ldt], zz[q], acc0);       // rows k + q >= D: the zeroed slack / z1 = 0
        acc1 = fma(Lc[(k + q) * ldt + 64], zz[q], acc1);
      }
    }
    // (the products are rounded before they are added - the oracle's arithmetic; the empty asm keeps them out of an fma)
    T s0 = se[l] * z2[l], s1 = se[l + 64] * z2[l + 64];
    asm volatile("" : "+v"(s0), "+v"(s1));
    if (l < D) p_ws[task * D + l] = acc0 + s0;
    if (row2) p_ws[task * D + l + 64] = acc1 + s1;
    __builtin_amdgcn_wave_barrier();
  }
}

// The same draws, one WAVE per task, the work matrix in registers (fp32, jitter on, D <= 8 NB).  The workgroup kernel above
// is bound by its LDS round trips: every trailing-update FMA reads its operands from LDS and writes its result back (1.5
// LDS operations per FMA, 2 workgroup barriers per panel, 3 tasks per CU: 53 us per task at D = 100).  Here lane
// (ty, tx) = (l >> 3, l & 7) owns the elements (ty + 8a, tx + 8b), b <= a, of the lower triangle (NB(NB+1)/2 VGPRs); only
// the current panel of 4 columns passes through LDS (one 16-byte row per lane in, one out), the rank-4 update reads 4
// panel values per block row / block column (16-byte loads) for 4 FMAs per owned element, there are no workgroup
// barriers, and the factor is never stored: p = L z is accumulated row by row as the panels finish (row r belongs to
// lane r & 63).  12+ tasks per CU.  Same streams and the same factor as rmhmc_momentum_kernel; the sums of p run in
// panel order.
template <int NB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(512 - kFusedWideVgprs))) void rmhmc_momentum_wave_kernel(const float* __restrict__ P, float jitter, int64_t C, int D,
                                                                 int n_traj, int traj_offset, uint64_t seed, uint64_t chain_offset,
                                                                 float* __restrict__ p_ws) {
  constexpr int NR = 8 * NB;                             // padded rows
  constexpr int NROW = (NR + 63) / 64;                   // rows per lane in the panel step
  __shared__ __attribute__((aligned(16))) float pan[NR * 4], pan2[NR * 4], zv[NR], evv[NR];
  const int l = threadIdx.x, ty = l >> 3, tx = l & 7;
  typedef float f4 __attribute__((ext_vector_type(4)));
  typedef float f2 __attribute__((ext_vector_type(2)));
  for (int e = l; e < NR * 4; e += 64) { pan[e] = 0.f; pan2[e] = 0.f; }
  const int64_t ntask = (int64_t)n_traj * C;
  for (int64_t task = blockIdx.x; task < ntask; task += gridDim.x) {
    const int t = (int)(task / C);
    const int64_t c = task - (int64_t)t * C;
    const uint64_t chain = chain_offset + (uint64_t)c;
    const uint32_t n = (uint32_t)(traj_offset + t);
    // ---- this task's matrix: W = P + diag(jitter u)  (S:113-116), lower blocks, straight from L2
    // (rows / columns >= D are clamped copies: a factor's leading D x D part does not depend on what lies beyond it, and
    //  nothing of the padding is stored.  P does not depend on the task: the compiler keeps these loads out of the task
    //  loop, i.e. P's share of a lane stays in VGPRs for the launch - 2 waves per SIMD at NB = 13)
    float W[NB][NB];
#pragma unroll
    for (int a = 0; a < NB; ++a) {
      const float* rowp = P + min(ty + 8 * a, D - 1) * D;
#pragma unroll
      for (int b = 0; b <= a; ++b) W[a][b] = rowp[min(tx + 8 * b, D - 1)];
    }
#pragma unroll
    for (int q = 0; q < NROW; ++q) {
      const int r = l + 64 * q;
      if (r < NR) {
        evv[r] = r < D ? jitter * uniform_elem<float>(seed, chain, n, PURPOSE_JITTER, 0, r) : 0.f;
        zv[r] = r < D ? normal_elem<float>(seed, chain, n, 0, r) : 0.f;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (ty == tx) {
#pragma unroll
      for (int a = 0; a < NB; ++a) W[a][a] += evv[ty + 8 * a];
    }
    float pacc[NROW];
#pragma unroll
    for (int q = 0; q < NROW; ++q) pacc[q] = 0.f;

    for (int bp = 0; bp < NB; ++bp) {
      if (8 * bp >= D) break;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int kb = 8 * bp + 4 * half;
        if (kb < D) {
          // ---- the panel's columns kb .. kb+3 (block column bp) leave their owners' registers
          if ((tx >> 2) == half) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
              if (b == bp) {                               // uniform: one of the NB bodies runs, register indices stay static
#pragma unroll
                for (int a = b; a < NB; ++a) pan[(ty + 8 * a) * 4 + (tx & 3)] = W[a][b];
              }
            }
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          // ---- diagonal block factor (every lane, registers), then the panel rows this lane handles
          float Ld[4][4], rinv[4];
#pragma unroll
          for (int cc = 0; cc < 4; ++cc) {
            const f4 rowv = *reinterpret_cast<const f4*>(pan + (kb + cc) * 4);
            const bool in = kb + cc < D;
#pragma unroll
            for (int c2 = 0; c2 < 4; ++c2) Ld[cc][c2] = (in && c2 <= cc) ? rowv[c2] : (cc == c2 ? 1.f : 0.f);
          }
#pragma unroll
          for (int cc = 0; cc < 4; ++cc) {
#pragma unroll
            for (int c2 = 0; c2 < cc; ++c2) {
              float v = Ld[cc][c2];
#pragma unroll
              for (int c3 = 0; c3 < c2; ++c3) v = fmaf(-Ld[cc][c3], Ld[c2][c3], v);
              Ld[cc][c2] = v * rinv[c2];
            }
            float v = Ld[cc][cc];
#pragma unroll
            for (int c3 = 0; c3 < cc; ++c3) v = fmaf(-Ld[cc][c3], Ld[cc][c3], v);
            rinv[cc] = fast_rsqrt<float>(v);
            Ld[cc][cc] = v * rinv[cc];
          }
          const f4 zk = *reinterpret_cast<const f4*>(zv + kb);
#pragma unroll
          for (int q = 0; q < NROW; ++q) {
            const int r = l + 64 * q;
            if (r < NR) {
              f4 out = {0.f, 0.f, 0.f, 0.f};
              if (r >= kb + 4) {
                const f4 wv = *reinterpret_cast<const f4*>(pan + r * 4);
                float lrow[4];
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                  float v = wv[cc];
#pragma unroll
                  for (int c3 = 0; c3 < cc; ++c3) v = fmaf(-lrow[c3], Ld[cc][c3], v);
                  lrow[cc] = v * rinv[cc];
                  pacc[q] = fmaf(lrow[cc], zk[cc], pacc[q]);
                }
                out = f4{lrow[0], lrow[1], lrow[2], lrow[3]};
              } else if (r >= kb) {                        // a row of the diagonal block: its finished entries times z
#pragma unroll
                for (int cc = 0; cc < 4; ++cc)
                  if (r == kb + cc) {
#pragma unroll
                    for (int c2 = 0; c2 <= cc; ++c2) pacc[q] = fmaf(Ld[cc][c2], zk[c2], pacc[q]);
                  }
              }
              if (r >= kb) *reinterpret_cast<f4*>(pan2 + r * 4) = out;      // rows of finished panels hold zeros: no-op updates
            }
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          // ---- rank-4 update of the owned blocks right of / below the panel
          // (block columns in chunks of CH: CH column vectors live at a time instead of NB)
          constexpr int CH = 4;
#pragma unroll
          for (int b0 = 0; b0 < NB; b0 += CH) {
            if (b0 + CH > bp) {
              f4 lj[CH];
#pragma unroll
              for (int u = 0; u < CH; ++u) lj[u] = (b0 + u < NB) ? *reinterpret_cast<const f4*>(pan2 + (tx + 8 * (b0 + u)) * 4) : f4{0.f, 0.f, 0.f, 0.f};
              f2 ljp[CH / 2][4];
#pragma unroll
              for (int u = 0; u < CH; u += 2)
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) ljp[u >> 1][cc] = f2{lj[u][cc], lj[u + 1][cc]};
#pragma unroll
              for (int a = b0; a < NB; ++a) {
                if (a >= bp) {
                  const f4 li = *reinterpret_cast<const f4*>(pan2 + (ty + 8 * a) * 4);
#pragma unroll
                  for (int u = 0; u < CH; u += 2) {        // two columns per v_pk_fma_f32 (columns left of the panel see zeros
                    if (b0 + u + 1 <= a) {                 //  in pan2: no-op updates)
                      f2 v = {W[a][b0 + u], W[a][b0 + u + 1]};
#pragma unroll
                      for (int cc = 0; cc < 4; ++cc) v = __builtin_elementwise_fma(f2{-li[cc], -li[cc]}, ljp[u >> 1][cc], v);
                      W[a][b0 + u] = v[0]; W[a][b0 + u + 1] = v[1];
                    } else if (b0 + u <= a) {
                      float v = W[a][b0 + u];
#pragma unroll
                      for (int cc = 0; cc < 4; ++cc) v = fmaf(-li[cc], lj[u][cc], v);
                      W[a][b0 + u] = v;
                    }
                  }
                }
              }
            }
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
#pragma unroll
    for (int q = 0; q < NROW; ++q) {
      const int r = l + 64 * q;
      if (r < D) p_ws[task * D + r] = pacc[q];
    }
    // pan2 holds zeros again except the last panel's diagonal rows (written as zeros above): nothing to clear
  }
}

// S = V0 diag(1 / lam0) V0^T from the eigen-system of the jitter-free P (one workgroup; once per run)
template <typename T>
__global__ void inverse_from_eigen_kernel(const T* __restrict__ V0, const T* __restrict__ lam0, T* __restrict__ S, int D) {
  for (int e = threadIdx.x; e < D * D; e += blockDim.x) {
    const int i = e / D, j = e - i * D;
    T acc = 0;
    for (int k = 0; k < D; ++k) acc = fma(V0[i * D + k] / lam0[k], V0[j * D + k], acc);
    S[e] = acc;
  }
}

}  // namespace hta
