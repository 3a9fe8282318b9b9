// Gaussian HMC, general D: one chain per 64-lane wave - the direct kernels, the eigenbasis route and its preparation kernels
// (included by hmc_gaussian.hip).
#pragma once
#include "common.hpp"
#include "philox.hpp"
#include "hmc_gaussian.hpp"

namespace hta {

// =============================================================================================
// general D: one chain per wave; lane l owns elements l + 64 r, r < R
// =============================================================================================
constexpr int GEN_WAVES = 4;

template <typename T, int R, int MASS> struct WaveModel {
  const T* P; const T* mu; const T* im; const T* mf; int D;
  T* bc;  // this wave's LDS broadcast buffer [64*R]
  T muv[R], imd[R];
  __device__ __forceinline__ void init(const GaussArgs<T>& a, T* lds, int lane) {
    P = a.P; mu = a.mu; im = a.inv_mass; mf = a.mass_factor; D = a.D; bc = lds;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = lane + 64 * r;
      muv[r] = j < D ? a.mu[j] : (T)0;
      imd[r] = (MASS == HTA_MASS_DIAG && j < D) ? a.inv_mass[j] : (T)1;
    }
  }
  // out_j = sum_k A[j][k] x_k for the lane's elements, A symmetric or accessed as A[k][j] (coalesced)
  // `tri`: only k <= j contributes (lower-triangular factor, accessed as A[j][k]).
  __device__ __forceinline__ void matvec(const T* __restrict__ A, const T (&x)[R], T (&out)[R], int lane,
                                         bool lower_tri) const {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) bc[lane + 64 * r] = x[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) out[r] = 0;
    if (!lower_tri) {
      for (int k = 0; k < D; ++k) {
        const T xk = bc[k];
        const T* row = A + (int64_t)k * D;  // A symmetric: A[k][j] == A[j][k]
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int j = lane + 64 * r;
          if (j < D) out[r] += row[j] * xk;
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int j = lane + 64 * r;
        if (j < D) {
          T acc = 0;
          for (int k = 0; k <= j; ++k) acc += A[(int64_t)j * D + k] * bc[k];
          out[r] = acc;
        }
      }
    }
  }
  __device__ __forceinline__ void vel(const T (&p)[R], T (&v)[R], int lane) const {
    if (MASS == HTA_MASS_FULL) { matvec(im, p, v, lane, false); return; }
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = (MASS == HTA_MASS_DIAG) ? imd[r] * p[r] : p[r];
  }
  __device__ __forceinline__ T curv(const T (&q)[R], T (&Pd)[R], int lane) const {
    T d[R];
#pragma unroll
    for (int r = 0; r < R; ++r) d[r] = (lane + 64 * r < D) ? q[r] - muv[r] : (T)0;
    matvec(P, d, Pd, lane, false);
    T quad = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) quad += d[r] * Pd[r];
    return (T)0.5 * wave_sum(quad);
  }
  __device__ __forceinline__ T kinetic(const T (&p)[R], int lane) const {
    T v[R]; vel(p, v, lane);
    T k = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) k += p[r] * v[r];
    return (T)0.5 * wave_sum(k);
  }
  template <bool REC = false>
  __device__ __forceinline__ T leapfrog(T (&q)[R], T (&p)[R], T (&Pd)[R], int L, T eps, int lane,
                                        T* rec_q = nullptr, T* rec_p = nullptr, int64_t rec_stride = 0) const {
    const T he = (T)0.5 * eps;
    T quad = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) p[r] -= he * Pd[r];
    for (int l = 0; l < L; ++l) {
      T v[R]; vel(p, v, lane);
#pragma unroll
      for (int r = 0; r < R; ++r) q[r] = q[r] + eps * v[r];
      quad = curv(q, Pd, lane);
#pragma unroll
      for (int r = 0; r < R; ++r) p[r] -= eps * Pd[r];
      if (REC) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int j = lane + 64 * r;
          if (j < D && rec_q) rec_q[l * rec_stride + j] = q[r];
          if (j < D && rec_p) rec_p[l * rec_stride + j] = p[r];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) p[r] += he * Pd[r];
    return quad;
  }
};

template <typename T, int R, int MASS>
__global__ __launch_bounds__(64 * GEN_WAVES) void hmc_gauss_wave_kernel(GaussArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T* lds = reinterpret_cast<T*>(smem_raw) + wave * 64 * R;
  const int64_t cc = (int64_t)blockIdx.x * GEN_WAVES + wave;
  const bool live = cc < a.C;
  const int64_t c = live ? cc : a.C - 1;  // dead waves shadow the last chain (barriers stay matched), no stores
  WaveModel<T, R, MASS> m;
  m.init(a, lds, lane);
  const int D = a.D;
  T th[R];
#pragma unroll
  for (int r = 0; r < R; ++r) th[r] = (lane + 64 * r < D) ? a.theta[c * D + lane + 64 * r] : (T)0;
  const uint64_t chain = a.chain_offset + (uint64_t)c;
  int32_t rejected = 0;

  for (int t = 0; t < a.n_traj; ++t) {
    const int n = a.traj_offset + t;
    T z[R], p[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = lane + 64 * r;
      z[r] = j < D ? normal_elem<T>(a.seed, chain, (uint32_t)n, 0, j) : (T)0;
    }
    if (MASS == HTA_MASS_FULL) m.matvec(a.mass_factor, z, p, lane, true);
    else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int j = lane + 64 * r;
        p[r] = (MASS == HTA_MASS_DIAG && j < D) ? a.mass_factor[j] * z[r] : z[r];
      }
    }
    T q[R], Pd[R];
#pragma unroll
    for (int r = 0; r < R; ++r) q[r] = th[r];
    const T quad0 = m.curv(q, Pd, lane);
    const T h_old = -(a.log_norm - quad0) + m.kinetic(p, lane);
    const T quad1 = m.leapfrog(q, p, Pd, a.L, a.eps, lane);
    const T logp1 = a.log_norm - quad1;
    const T h_new = -logp1 + m.kinetic(p, lane);
    const T u = u23<T>(philox_block(a.seed, chain, (uint32_t)n, PURPOSE_MH, 0, 0).x);
    const bool acc = mh_accept<T>(h_old, h_new, logp1, u);
    if (acc) {
#pragma unroll
      for (int r = 0; r < R; ++r) th[r] = q[r];
    } else {
      ++rejected;
      if (n == a.burn + 1) {
#pragma unroll
        for (int r = 0; r < R; ++r) if (lane + 64 * r < D) th[r] = a.theta_init[c * D + lane + 64 * r];
      }
    }
    if (live) {
      if (a.samples && n > a.burn) {
        T* row = a.samples + ((int64_t)(n - a.burn) * a.C + c) * D;
#pragma unroll
        for (int r = 0; r < R; ++r) if (lane + 64 * r < D) row[lane + 64 * r] = th[r];
      }
      if (lane == 0) {
        if (a.H_old) a.H_old[(int64_t)t * a.C + c] = h_old;
        if (a.H_new) a.H_new[(int64_t)t * a.C + c] = h_new;
        if (a.accept) a.accept[(int64_t)t * a.C + c] = acc ? 1 : 0;
      }
    }
  }
  if (live) {
#pragma unroll
    for (int r = 0; r < R; ++r) if (lane + 64 * r < D) a.theta[c * D + lane + 64 * r] = th[r];
    if (lane == 0 && a.reject_count) a.reject_count[c] += rejected;
  }
}


// =============================================================================================
// general D, identity mass: the wave-per-chain kernel in the eigenbasis of P
//
// Same change of variables as the small-D route: y = Q^T (q - mu), r = Q^T p decouple the leapfrog map by coordinate, so a
// step is two multiply-adds per element and no matrix-vector product at all (the direct kernel streams P once per step).
// What is left per trajectory are two products with the D x D eigenvector matrix: the rotation of the momentum draw
// (r = Q^T z: the same Philox normals as the direct kernel) and the sample row q = mu + Q y.  P is diagonalised once per
// launch by the Jacobi kernel of the RMHMC path (csrc/rmhmc_metric.hip: one workgroup, A and V in LDS; D <= ~140 fp32 /
// ~99 fp64), in float32 polished (eig_polish_kernel below: one more launch of D blocks, D^3 multiply-adds), then transposed once.  Eig area (workspace): V[D][D] (V[i][k] = component i of eigenvector k) | Vt[D][D] | lam[D].
// =============================================================================================
template <typename T>
__global__ void transpose_kernel(const T* __restrict__ V, T* __restrict__ Vt, int D) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < D * D; e += gridDim.x * blockDim.x) {
    const int i = e / D, k = e - i * D;
    Vt[k * D + i] = V[e];
  }
}

// The Jacobi kernel rotates in T: in float32 its ~8 D rotations per column leave every column of V short by the same sign (|v|^2 - 1 =
// -1e-6 at D = 63 ... 128, off-diagonal V^T V at rounding level), which 0.5 |V^T z|^2 and 0.5 sum lam y^2 carry into H_old and H_new
// alike (1e-4 at |H| = 100; the difference, and so every decision, does not see it).  One block per column k: v_k <- v_k / |v_k| and
// lam_k <- v_k^T P v_k / |v_k|^2, sums in double.
template <typename T>
__global__ __launch_bounds__(128) void eig_polish_kernel(const T* __restrict__ P, T* __restrict__ V, T* __restrict__ lam, int D) {
  __shared__ double red[2][128];
  const int k = blockIdx.x;
  double nn = 0, rq = 0;
  for (int i = threadIdx.x; i < D; i += blockDim.x) {
    const double vi = (double)V[(int64_t)i * D + k];
    double w = 0;
    for (int j = 0; j < D; ++j) w += (double)P[(int64_t)i * D + j] * (double)V[(int64_t)j * D + k];
    nn += vi * vi;
    rq += vi * w;
  }
  red[0][threadIdx.x] = nn; red[1][threadIdx.x] = rq;
  __syncthreads();
  for (int h = 64; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) { red[0][threadIdx.x] += red[0][threadIdx.x + h]; red[1][threadIdx.x] += red[1][threadIdx.x + h]; }
    __syncthreads();
  }
  nn = red[0][0]; rq = red[1][0];
  if (!(nn > 0)) return;                 // (block-uniform: a non-finite or empty column is left as the Jacobi kernel wrote it)
  const double sc = 1.0 / sqrt(nn);
  for (int i = threadIdx.x; i < D; i += blockDim.x) V[(int64_t)i * D + k] = (T)((double)V[(int64_t)i * D + k] * sc);
  if (threadIdx.x == 0) lam[k] = (T)(rq / nn);
}

template <typename T, int R>
__global__ __launch_bounds__(64 * GEN_WAVES) void hmc_gauss_wave_eig_kernel(GaussArgs<T> a, const T* __restrict__ eig) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T* lds = reinterpret_cast<T*>(smem_raw) + wave * 64 * R;
  const int64_t cc = (int64_t)blockIdx.x * GEN_WAVES + wave;
  const bool live = cc < a.C;
  const int64_t c = live ? cc : a.C - 1;  // dead waves shadow the last chain (barriers stay matched), no stores
  WaveModel<T, R, HTA_MASS_NONE> m;
  m.init(a, lds, lane);
  const int D = a.D;
  const T* V = eig;                       // matvec(V, x) = V^T x  (it reads A[k][j])
  const T* Vt = eig + (int64_t)D * D;     // matvec(Vt, x) = V x
  const T* lamp = Vt + (int64_t)D * D;
  const T eps = a.eps, he = (T)0.5 * a.eps;
  T lam[R], nel[R], hl[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int j = lane + 64 * r;
    lam[r] = j < D ? lamp[j] : (T)0;
    nel[r] = -(eps * lam[r]); hl[r] = he * lam[r];
  }
  auto to_y = [&](const T* __restrict__ q, T (&y)[R]) {        // every wave of the workgroup must call this together
    T d[R];
#pragma unroll
    for (int r = 0; r < R; ++r) d[r] = (lane + 64 * r < D) ? q[c * D + lane + 64 * r] - m.muv[r] : (T)0;
    m.matvec(V, d, y, lane, false);
  };
  auto to_q = [&](const T (&y)[R], T (&q)[R]) {                // likewise
    m.matvec(Vt, y, q, lane, false);
#pragma unroll
    for (int r = 0; r < R; ++r) q[r] += m.muv[r];
  };
  auto potential = [&](const T (&y)[R]) {
    T s = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) s = fma(lam[r] * y[r], y[r], s);
    return (T)0.5 * wave_sum(s);
  };
  auto kinetic = [&](const T (&p)[R]) {
    T s = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) s = fma(p[r], p[r], s);
    return (T)0.5 * wave_sum(s);
  };
  T yc[R], qc[R];                // qc: the current point as it is stored (a rejection repeats it bit for bit, S:1018)
#pragma unroll
  for (int r = 0; r < R; ++r) qc[r] = (lane + 64 * r < D) ? a.theta[c * D + lane + 64 * r] : (T)0;
  to_y(a.theta, yc);
  T quadc = potential(yc);
  const uint64_t chain = a.chain_offset + (uint64_t)c;
  int32_t rejected = 0;

  for (int t = 0; t < a.n_traj; ++t) {
    const int n = a.traj_offset + t;
    T z[R], p[R], y[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = lane + 64 * r;
      z[r] = j < D ? normal_elem<T>(a.seed, chain, (uint32_t)n, 0, j) : (T)0;      // S:185-186
    }
    m.matvec(V, z, p, lane, false);                                                  // r = Q^T z
    const T h_old = -(a.log_norm - quadc) + kinetic(p);                              // S:971
#pragma unroll
    for (int r = 0; r < R; ++r) { y[r] = yc[r]; p[r] = fma(-hl[r], yc[r], p[r]); }  // S:281
    for (int l = 0; l < a.L; ++l) {                                                  // S:283-298
#pragma unroll
      for (int r = 0; r < R; ++r) { y[r] = fma(eps, p[r], y[r]); p[r] = fma(nel[r], y[r], p[r]); }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) p[r] = fma(hl[r], y[r], p[r]);                      // S:302
    const T quad1 = potential(y);
    const T logp1 = a.log_norm - quad1;
    const T h_new = -logp1 + kinetic(p);                                             // S:995
    const T u = u23<T>(philox_block(a.seed, chain, (uint32_t)n, PURPOSE_MH, 0, 0).x);
    const bool acc = mh_accept<T>(h_old, h_new, logp1, u);                           // S:1000-1004
    T yinit[R], qp[R];
    if (n == a.burn + 1) to_y(a.theta_init, yinit);          // workgroup-uniform: the Q2 candidate of every chain
    to_q(y, qp);                                              // workgroup-uniform: the proposal mapped back
    if (acc) {
#pragma unroll
      for (int r = 0; r < R; ++r) { yc[r] = y[r]; qc[r] = qp[r]; }
      quadc = quad1;
    } else {
      ++rejected;
      if (n == a.burn + 1) {                                  // Q2 reset (S:1016-1018): params_init itself
#pragma unroll
        for (int r = 0; r < R; ++r) {
          yc[r] = yinit[r];
          qc[r] = (lane + 64 * r < D) ? a.theta_init[c * D + lane + 64 * r] : (T)0;
        }
        quadc = potential(yc);
      }
    }
    if (a.samples && n > a.burn && live) {
      T* row = a.samples + ((int64_t)(n - a.burn) * a.C + c) * D;
#pragma unroll
      for (int r = 0; r < R; ++r) if (lane + 64 * r < D) row[lane + 64 * r] = qc[r];
    }
    if (live && lane == 0) {
      if (a.H_old) a.H_old[(int64_t)t * a.C + c] = h_old;
      if (a.H_new) a.H_new[(int64_t)t * a.C + c] = h_new;
      if (a.accept) a.accept[(int64_t)t * a.C + c] = acc ? 1 : 0;
    }
  }
  if (live) {
#pragma unroll
    for (int r = 0; r < R; ++r) if (lane + 64 * r < D) a.theta[c * D + lane + 64 * r] = qc[r];
    if (lane == 0 && a.reject_count) a.reject_count[c] += rejected;
  }
}

template <typename T, int R, int MASS>
__global__ __launch_bounds__(64 * GEN_WAVES) void leapfrog_gauss_wave_kernel(GaussArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T* lds = reinterpret_cast<T*>(smem_raw) + wave * 64 * R;
  const int64_t cc = (int64_t)blockIdx.x * GEN_WAVES + wave;
  const bool live = cc < a.C;
  const int64_t c = live ? cc : a.C - 1;
  WaveModel<T, R, MASS> m;
  m.init(a, lds, lane);
  const int D = a.D;
  T q[R], p[R], Pd[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int j = lane + 64 * r;
    q[r] = j < D ? a.theta[c * D + j] : (T)0;
    p[r] = j < D ? a.p_io[c * D + j] : (T)0;
  }
  m.curv(q, Pd, lane);
  m.template leapfrog<true>(q, p, Pd, a.L, a.eps, lane, (live && a.path_theta) ? a.path_theta + c * D : nullptr,
                            (live && a.path_p) ? a.path_p + c * D : nullptr, a.C * D);
  if (live) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = lane + 64 * r;
      if (j < D) {
        a.theta[c * D + j] = q[r]; a.p_io[c * D + j] = p[r];
        if (a.path_p && a.L > 0) a.path_p[((int64_t)(a.L - 1) * a.C + c) * D + j] = p[r];
      }
    }
  }
}

}  // namespace hta
