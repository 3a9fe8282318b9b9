// Gaussian HMC, small D: one chain per lane - the direct kernels and their eigenbasis route (included by hmc_gaussian.hip).
#pragma once
#include <type_traits>
#include <utility>
#include "common.hpp"
#include "philox.hpp"
#include "hmc_gaussian.hpp"

namespace hta {

// =============================================================================================
// small-D: thread per chain
//
// What bounds it (measured, tools/scratch/issue_bench.hip -> profiles/r01_issue_bench.txt): at
// BASELINE config 2 (1024 chains x D=3) the launch is 16 waves on a 1024-SIMD chip, and ONE wave
// issues a dependent VALU instruction only every ~2-2.5 ns and pays ~14 ns per taken loop branch.
// Time per leapfrog step is therefore (instructions per step per wave), not bytes and not flops.
// So the inner loop is written for the fewest instructions per step:
//   * d = q - mu and pre-scaled wave-uniform operands: d <- d + (eps M^-1) p ; p <- p + (-eps P) d,
//     i.e. D + D*D fused multiply-adds, the kick accumulating straight into p (S:283-298);
//   * fp32: two elements per instruction (v_pk_fma_f32 on explicit float2 pairs): 8 instead of 12
//     instructions per step at D=3 (15.8 vs 22.8 ns/step);
//   * steps in straight-line blocks of 10 and 5 (repeat_steps; the reference's L values are multiples of 5): L = 25 is
//     two back-edges per trajectory;
//   * P d is formed only at trajectory end points, and the potential at the current point is
//     carried from the previous trajectory (accepted -> end point, rejected -> unchanged).
// Rejected alternatives (same microbenchmark): one chain per DPP quad (4 instead of 12 FMAs per
// step, but a DPP read of a just-written register costs ~7.6 ns: 23-28 ns/step); half-filled waves
// (slower: 30.9 ns/step); two chains per lane (no gain).
//
// Random numbers.  With a workspace the momentum normals and log-uniforms of every trajectory of
// the launch are produced first by a full-chip kernel (rng_fill_small_kernel: one thread per
// (trajectory, chain), ~1e6 threads for config 2) as 16-byte records [z_0..z_{D-1}, log u, pad] and
// the trajectory kernel loads one record per trajectory, one trajectory ahead: ~2.5k cycles of
// Philox/Box-Muller per trajectory leave the 16 busy SIMDs for the 1000 idle ones.  Without a
// workspace the draws are made inline.  Same Philox stream either way.
// =============================================================================================
// eig block of the eigenbasis route (see eig_small_kernel): offsets of Qt, Tin, Tout behind lam[D]
constexpr int EIG_ELEMS = 128;
#define EIG_QT(D) (D)
#define EIG_TIN(D) ((D) + (D) * (D))
#define EIG_TOUT(D) ((D) + 2 * (D) * (D))

typedef float f2 __attribute__((ext_vector_type(2)));

template <typename T> struct RecVec;
template <> struct RecVec<float> { typedef float type __attribute__((ext_vector_type(4))); static constexpr int N = 4; };
template <> struct RecVec<double> { typedef double type __attribute__((ext_vector_type(2))); static constexpr int N = 2; };
// elements per (trajectory, chain) record: D normals + log u, padded to 16-byte vectors
template <typename T, int D> constexpr int rec_elems() { return ((D + 1 + RecVec<T>::N - 1) / RecVec<T>::N) * RecVec<T>::N; }

// L leapfrog steps for a lone wave: a taken branch costs ~14 ns (six dependent FMAs), so the steps come in straight-line
// blocks of 25; what is left over (blocks of 10, one of 5, single steps) sits off the hot path.  L = 25, 50, ... take no
// branch inside a trajectory at all.
template <typename F> __device__ __forceinline__ void repeat_steps(int L, F&& step) {
  int l = L;
  while (l >= 25) {
#pragma unroll
    for (int u = 0; u < 25; ++u) step();
    l -= 25;
  }
  if (__builtin_expect(l > 0, 0)) {
    while (l >= 10) {
#pragma unroll
      for (int u = 0; u < 10; ++u) step();
      l -= 10;
    }
    if (l >= 5) {
#pragma unroll
      for (int u = 0; u < 5; ++u) step();
      l -= 5;
    }
    while (l > 0) { step(); --l; }
  }
}

template <typename T, int D, int MASS> struct SmallModel {
  static constexpr int NM = MASS == HTA_MASS_FULL ? D * D : (MASS == HTA_MASS_DIAG ? D : 1);
  T P[D][D]; T nEP[D][D]; T mu[D]; T im[NM]; T eIM[NM]; T mf[NM]; T eps;
  __device__ __forceinline__ void load(const GaussArgs<T>& a, bool need_mf) {
    eps = a.eps;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      mu[i] = a.mu[i];
#pragma unroll
      for (int j = 0; j < D; ++j) { P[i][j] = a.P[i * D + j]; nEP[i][j] = -(a.eps * P[i][j]); }
    }
    if (MASS != HTA_MASS_NONE) {
#pragma unroll
      for (int i = 0; i < NM; ++i) {
        im[i] = a.inv_mass[i]; eIM[i] = a.eps * im[i];
        mf[i] = need_mf ? a.mass_factor[i] : (T)0;
      }
    }
  }
  // v = M^-1 p
  __device__ __forceinline__ void vel(const T (&p)[D], T (&v)[D]) const {
#pragma unroll
    for (int i = 0; i < D; ++i) {
      if (MASS == HTA_MASS_NONE) v[i] = p[i];
      else if (MASS == HTA_MASS_DIAG) v[i] = im[i] * p[i];
      else { T acc = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) acc += im[i * D + k] * p[k];
        v[i] = acc; }
    }
  }
  // Pd = P d;  returns 0.5 d^T P d
  __device__ __forceinline__ T curv_d(const T (&d)[D], T (&Pd)[D]) const {
    T quad = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      T acc = P[i][0] * d[0];
#pragma unroll
      for (int k = 1; k < D; ++k) acc += P[i][k] * d[k];
      Pd[i] = acc;
      quad += d[i] * acc;
    }
    return (T)0.5 * quad;
  }
  __device__ __forceinline__ T kinetic(const T (&p)[D]) const {
    T v[D]; vel(p, v);
    T k = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) k += p[i] * v[i];
    return (T)0.5 * k;
  }
  // one full step on (d, p): drift then kick (S:283-298), scalar form
  __device__ __forceinline__ void step(T (&d)[D], T (&p)[D]) const {
#pragma unroll
    for (int i = 0; i < D; ++i) {
      if (MASS == HTA_MASS_NONE) d[i] = fma(eps, p[i], d[i]);
      else if (MASS == HTA_MASS_DIAG) d[i] = fma(eIM[i], p[i], d[i]);
      else { T acc = d[i];
#pragma unroll
        for (int k = 0; k < D; ++k) acc = fma(eIM[i * D + k], p[k], acc);
        d[i] = acc; }
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
#pragma unroll
      for (int i = 0; i < D; ++i) p[i] = fma(nEP[i][k], d[k], p[i]);
    }
  }
  // L steps.  fp32: the same FMAs as step(), two elements per v_pk_fma_f32 (bitwise identical results).
  __device__ __forceinline__ void run_steps(T (&d)[D], T (&p)[D], int L) const {
    if constexpr (sizeof(T) == 4 && D >= 2) {
      constexpr int NP = D / 2;
      constexpr bool R = (D & 1) != 0;
      f2 dP[NP], pP[NP], AP[D][NP], EP[MASS == HTA_MASS_FULL ? D : 1][NP];
      float dS = 0, pS = 0, AS[D], ES[MASS == HTA_MASS_FULL ? D : 1];
#pragma unroll
      for (int j = 0; j < NP; ++j) { dP[j] = f2{d[2 * j], d[2 * j + 1]}; pP[j] = f2{p[2 * j], p[2 * j + 1]}; }
      if (R) { dS = d[D - 1]; pS = p[D - 1]; }
#pragma unroll
      for (int k = 0; k < D; ++k) {              // column k of -eps P (and of eps M^-1 for a full mass)
#pragma unroll
        for (int j = 0; j < NP; ++j) AP[k][j] = f2{nEP[2 * j][k], nEP[2 * j + 1][k]};
        AS[k] = R ? nEP[D - 1][k] : 0.f;
        if (MASS == HTA_MASS_FULL) {
#pragma unroll
          for (int j = 0; j < NP; ++j) EP[k][j] = f2{eIM[(2 * j) * D + k], eIM[(2 * j + 1) * D + k]};
          ES[k] = R ? eIM[(D - 1) * D + k] : 0.f;
        }
      }
      f2 eP[NP]; float eS = eps;
#pragma unroll
      for (int j = 0; j < NP; ++j)
        eP[j] = (MASS == HTA_MASS_DIAG) ? f2{eIM[2 * j], eIM[2 * j + 1]} : f2{eps, eps};
      if (MASS == HTA_MASS_DIAG && R) eS = eIM[D - 1];
      repeat_steps(L, [&]() {
        if (MASS == HTA_MASS_FULL) {
          f2 nd[NP]; float ndS = dS;
#pragma unroll
          for (int j = 0; j < NP; ++j) nd[j] = dP[j];
#pragma unroll
          for (int k = 0; k < D; ++k) {
            const float pk = (k < 2 * NP) ? pP[k / 2][k % 2] : pS;
#pragma unroll
            for (int j = 0; j < NP; ++j) nd[j] = __builtin_elementwise_fma(EP[k][j], f2{pk, pk}, nd[j]);
            if (R) ndS = fmaf(ES[k], pk, ndS);
          }
#pragma unroll
          for (int j = 0; j < NP; ++j) dP[j] = nd[j];
          dS = ndS;
        } else {
#pragma unroll
          for (int j = 0; j < NP; ++j) dP[j] = __builtin_elementwise_fma(eP[j], pP[j], dP[j]);
          if (R) dS = fmaf(eS, pS, dS);
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const float dk = (k < 2 * NP) ? dP[k / 2][k % 2] : dS;
#pragma unroll
          for (int j = 0; j < NP; ++j) pP[j] = __builtin_elementwise_fma(AP[k][j], f2{dk, dk}, pP[j]);
          if (R) pS = fmaf(AS[k], dk, pS);
        }
      });
#pragma unroll
      for (int j = 0; j < NP; ++j) { d[2 * j] = dP[j].x; d[2 * j + 1] = dP[j].y; p[2 * j] = pP[j].x; p[2 * j + 1] = pP[j].y; }
      if (R) { d[D - 1] = dS; p[D - 1] = pS; }
    } else {
      repeat_steps(L, [&]() { step(d, p); });
    }
  }
  // leapfrog (S:281-302) on d = q - mu.  Pd: in = P d at the start, out = P d at the end.
  // Returns 0.5 d^T P d at the end point.
  template <bool REC = false>
  __device__ __forceinline__ T leapfrog(T (&d)[D], T (&p)[D], T (&Pd)[D], int L, T* rec_q = nullptr,
                                        T* rec_p = nullptr, int64_t rec_stride = 0) const {
    const T he = (T)0.5 * eps;
#pragma unroll
    for (int i = 0; i < D; ++i) p[i] -= he * Pd[i];                 // S:281
    if (REC) {
      for (int l = 0; l < L; ++l) {
        step(d, p);                                                  // S:283-298
#pragma unroll
        for (int i = 0; i < D; ++i) {                                // S:299-300
          if (rec_q) rec_q[l * rec_stride + i] = d[i] + mu[i];
          if (rec_p) rec_p[l * rec_stride + i] = p[i];
        }
      }
    } else {
      run_steps(d, p, L);
    }
    const T quad = curv_d(d, Pd);
#pragma unroll
    for (int i = 0; i < D; ++i) p[i] += he * Pd[i];                 // S:302
    return quad;
  }
};

// draws of one trajectory for one chain: D normals + log(u)
template <typename T, int D>
__device__ __forceinline__ void draw_inline(uint64_t seed, uint64_t chain, uint32_t n, T (&z)[D], T& logu) {
  constexpr int NQ = (D + 3) / 4;
#pragma unroll
  for (int b = 0; b < NQ; ++b) {
    T zz[4];
    normal4<T>(philox_block(seed, chain, n, PURPOSE_MOMENTUM, 0, b), zz);
#pragma unroll
    for (int i = 0; i < 4; ++i) if (4 * b + i < D) z[4 * b + i] = zz[i];
  }
  logu = log(u23<T>(philox_block(seed, chain, n, PURPOSE_MH, 0, 0).x));
}

// workspace: record [t][c] of rec_elems<T,D>() values = (z_0 .. z_{D-1}, log u, padding)
template <typename T, int D>
__global__ void rng_fill_small_kernel(T* __restrict__ ws, int64_t C, int n_traj, int traj_offset, uint64_t seed,
                                      uint64_t chain_offset, const T* __restrict__ eig, T lu_scale) {
  constexpr int W = rec_elems<T, D>();
  T Q[D][D];            // eigenbasis route: records hold Q^T z (wave-uniform operands); eig block: Qt[k][i] = Q[i][k]
  if (eig) {
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int k = 0; k < D; ++k) Q[i][k] = eig[EIG_QT(D) + k * D + i];
  }
  typedef typename RecVec<T>::type V;
  const int64_t total = C * n_traj;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = idx / C, c = idx - t * C;
    T rec[W];
#pragma unroll
    for (int i = 0; i < W; ++i) rec[i] = 0;
    T z[D], lu;
    draw_inline<T, D>(seed, chain_offset + (uint64_t)c, (uint32_t)(traj_offset + (int)t), z, lu);
    if (eig) {
#pragma unroll
      for (int k = 0; k < D; ++k) {
        T acc = Q[0][k] * z[0];
#pragma unroll
        for (int i = 1; i < D; ++i) acc = fma(Q[i][k], z[i], acc);
        rec[k] = acc;
      }
    } else {
#pragma unroll
      for (int j = 0; j < D; ++j) rec[j] = z[j];
    }
    rec[D] = lu_scale * lu;          // the quad kernel compares doubled energies: it gets 2 log u
    V* out = reinterpret_cast<V*>(ws + idx * W);
#pragma unroll
    for (int i = 0; i < W / RecVec<T>::N; ++i) {
      V v;
#pragma unroll
      for (int e = 0; e < RecVec<T>::N; ++e) v[e] = rec[i * RecVec<T>::N + e];
      out[i] = v;
    }
  }
}

template <typename T, int D>
__device__ __forceinline__ void load_record(const T* __restrict__ ws, size_t rec_index, T (&z)[D], T& logu) {
  constexpr int W = rec_elems<T, D>();
  typedef typename RecVec<T>::type V;
  const V* in = reinterpret_cast<const V*>(ws + rec_index * W);
  T rec[W];
#pragma unroll
  for (int i = 0; i < W / RecVec<T>::N; ++i) {
    const V v = in[i];
#pragma unroll
    for (int e = 0; e < RecVec<T>::N; ++e) rec[i * RecVec<T>::N + e] = v[e];
  }
#pragma unroll
  for (int j = 0; j < D; ++j) z[j] = rec[j];
  logu = rec[D];
}

template <typename T, int D, int MASS, bool WS, bool DIAG>
__global__ __launch_bounds__(256) void hmc_gauss_small_kernel(GaussArgs<T> a) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= a.C) return;
  SmallModel<T, D, MASS> m;
  m.load(a, true);
  const size_t C = (size_t)a.C;
  T th[D], dc[D], Pdc[D];
#pragma unroll
  for (int i = 0; i < D; ++i) { th[i] = a.theta[c * D + i]; dc[i] = th[i] - m.mu[i]; }
  T quadc = m.curv_d(dc, Pdc);        // potential state at the current point, carried across trajectories
  const uint64_t chain = a.chain_offset + (uint64_t)c;
  const T he = (T)0.5 * m.eps;
  int32_t rejected = 0;

  T z[D], logu = 0;
  const T* rec = a.ws_z + (size_t)c * rec_elems<T, D>();   // this chain's record of trajectory t (+1 row of slack)
  const size_t rec_step = C * rec_elems<T, D>();
  if (WS) load_record<T, D>(rec, 0, z, logu);
  // Sample rows.  CDNA's vmcnt counts stores as well as loads, and the compiler sizes the wait for the
  // pre-fetched record by the path with the FEWEST memory operations behind it.  So every trajectory
  // issues exactly D stores (to its sample row, or -- while n <= burn / no sample buffer -- to this
  // chain's slot of `theta`, which is rewritten at the end anyway), and the same D stores are issued
  // once before the loop: the wait then becomes vmcnt(D+1) on every path instead of stalling each
  // trajectory on the previous trajectory's stores (~350 ns, profiles/r01_cfg2_*).
  T* const scratch_row = a.theta + c * D;
  T* srow = a.samples ? a.samples + ((size_t)(a.traj_offset > a.burn ? a.traj_offset - a.burn : 1) * C + c) * D
                      : scratch_row;
  const size_t srow_step = a.samples ? C * D : 0;
#pragma unroll
  for (int i = 0; i < D; ++i) scratch_row[i] = th[i];
  for (int t = 0; t < a.n_traj; ++t) {
    const int n = a.traj_offset + t;
    T zn[D], logun = 0;
    if (WS) {          // next trajectory's draws: issued now, consumed after this trajectory's leapfrog
      rec += rec_step;
      load_record<T, D>(rec, 0, zn, logun);
    } else {
      draw_inline<T, D>(a.seed, chain, (uint32_t)n, z, logu);
    }
    // ---- gibbs: p ~ N(0, M)  (S:185-202)
    T p[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      if (MASS == HTA_MASS_NONE) p[i] = z[i];
      else if (MASS == HTA_MASS_DIAG) p[i] = m.mf[i] * z[i];
      else { T acc = 0;
#pragma unroll
        for (int k = 0; k <= i; ++k) acc += m.mf[i * D + k] * z[k];
        p[i] = acc; }
    }
    // ---- H_old (S:971)
    const T h_old = -(a.log_norm - quadc) + m.kinetic(p);
    // ---- leapfrog (S:973)
    T d[D], Pd[D];
#pragma unroll
    for (int i = 0; i < D; ++i) { d[i] = dc[i]; p[i] -= he * Pdc[i]; }   // S:281
    m.run_steps(d, p, a.L);                                                // S:283-298
    const T quad1 = m.curv_d(d, Pd);
#pragma unroll
    for (int i = 0; i < D; ++i) p[i] += he * Pd[i];                       // S:302
    // ---- H_new (S:995), MH (S:1000-1004)
    const T logp1 = a.log_norm - quad1;
    const T h_new = -logp1 + m.kinetic(p);
    const bool acc = mh_accept_logu<T>(h_old, h_new, logp1, logu);
    // ---- bookkeeping (S:1007-1026; Q2 reset at n == burn+1)
    rejected += acc ? 0 : 1;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      th[i] = acc ? d[i] + m.mu[i] : th[i];
      dc[i] = acc ? d[i] : dc[i];
      Pdc[i] = acc ? Pd[i] : Pdc[i];
    }
    quadc = acc ? quad1 : quadc;
    if (n == a.burn + 1 && !acc) {
#pragma unroll
      for (int i = 0; i < D; ++i) { th[i] = a.theta_init[c * D + i]; dc[i] = th[i] - m.mu[i]; }
      quadc = m.curv_d(dc, Pdc);
    }
    {
      const bool keep = n > a.burn;
      T* dst = keep ? srow : scratch_row;
#pragma unroll
      for (int i = 0; i < D; ++i) dst[i] = th[i];
      srow += keep ? srow_step : 0;
    }
    if (DIAG) {
      if (a.H_old) a.H_old[(size_t)t * C + c] = h_old;
      if (a.H_new) a.H_new[(size_t)t * C + c] = h_new;
      if (a.accept) a.accept[(size_t)t * C + c] = acc ? 1 : 0;
    }
    if (WS) {
#pragma unroll
      for (int j = 0; j < D; ++j) z[j] = zn[j];
      logu = logun;
    }
  }
#pragma unroll
  for (int i = 0; i < D; ++i) a.theta[c * D + i] = th[i];
  if (a.reject_count) a.reject_count[c] += rejected;
}


// =============================================================================================
// small-D, identity mass: the same trajectories integrated in the eigenbasis of P
//
// With M = I the Hamiltonian is invariant under y = Q^T (q - mu), r = Q^T p for the orthogonal Q of
// P = Q diag(lam) Q^T, and in (y, r) the leapfrog map (S:281-302) decouples by coordinate:
//     r_i -= eps lam_i y_i ;  y_i += eps r_i          -> 2 D fused multiply-adds per step instead of D + D*D.
// At config 2 (D = 3, one 64-chain wave per CU, issue bound) that is 4 instead of 8 VALU instructions per step.
// eig_small_kernel diagonalises P once per launch (one thread, cyclic Jacobi in fp64, registers only), the
// pre-draw pass rotates the momentum normals (r = Q^T z: the records still come from the same Philox draws),
// energies are 0.5 sum lam_i y_i^2 + 0.5 |r|^2, and a sample row is q = mu + Q y.  Same map, same draws, same
// accept rule as the direct kernel above; results differ from it by rounding only (tests compare both routes).
// =============================================================================================
// Layout of the eig block (T, EIG_ELEMS elements): lam[D] | Qt[D][D] (rotation of the draws, r = Qt z) | Tin[D][D]
// (y = Tin (q - mu)) | Tout[D][D] (q = mu + Tout y).
// A mass matrix M = L L^T (diag or full; `mass_factor` is L, S:199-201) is whitened away first: with d~ = L^T d,
// p~ = L^-1 p the leapfrog map with mass M is the identity-mass map for P~ = L^-1 P L^-T, the momentum draw p = L z
// (S:198-201) is p~ = z and the kinetic energy is 0.5 |p~|^2.  So: P~ = Q diag(lam) Q^T, Qt = Q^T, Tin = Q^T L^T,
// Tout = L^-T Q.  Identity mass: L = I.

template <typename T, int D>
__global__ void eig_small_kernel(const T* __restrict__ P, int mass_kind, const T* __restrict__ mass_factor,
                                 T* __restrict__ eig) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double A[D][D], V[D][D], Lm[D][D], Li[D][D];
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      A[i][j] = 0.5 * ((double)P[i * D + j] + (double)P[j * D + i]);   // the precision matrix is symmetric
      V[i][j] = i == j ? 1.0 : 0.0;
      Lm[i][j] = mass_kind == HTA_MASS_NONE ? (i == j ? 1.0 : 0.0)
                 : mass_kind == HTA_MASS_DIAG ? (i == j ? (double)mass_factor[i] : 0.0)
                                              : (j <= i ? (double)mass_factor[i * D + j] : 0.0);
      Li[i][j] = 0.0;
    }
  if (mass_kind != HTA_MASS_NONE) {
    // Li = L^-1 (lower triangular, forward substitution), then A <- Li A Li^T
#pragma unroll
    for (int j = 0; j < D; ++j) {
      Li[j][j] = 1.0 / Lm[j][j];
#pragma unroll
      for (int i = 0; i < D; ++i) {
        if (i > j) {
          double acc = 0;
#pragma unroll
          for (int k = 0; k < D; ++k) if (k >= j && k < i) acc += Lm[i][k] * Li[k][j];
          Li[i][j] = -acc / Lm[i][i];
        }
      }
    }
    double B[D][D];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) {
        double acc = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) acc += Li[i][k] * A[k][j];
        B[i][j] = acc;
      }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) {
        double acc = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) acc += B[i][k] * Li[j][k];
        A[i][j] = acc;
      }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) if (i < j) { const double m = 0.5 * (A[i][j] + A[j][i]); A[i][j] = A[j][i] = m; }
  } else {
#pragma unroll
    for (int i = 0; i < D; ++i) Li[i][i] = 1.0;
  }
  for (int sweep = 0; sweep < 12; ++sweep) {
    double off = 0, dia = 0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) { if (i < j) off += A[i][j] * A[i][j]; if (i == j) dia += A[i][i] * A[i][i]; }
    if (!(off > 1e-34 * dia)) break;
#pragma unroll
    for (int p = 0; p < D - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < D; ++q) {
        const double apq = A[p][q];
        if (fabs(apq) > 1e-300) {
          const double tau = (A[q][q] - A[p][p]) / (2.0 * apq);
          const double t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
          const double c = 1.0 / sqrt(1.0 + t * t), sn = t * c;
#pragma unroll
          for (int k = 0; k < D; ++k) {       // A <- A J (columns p, q)
            const double akp = A[k][p], akq = A[k][q];
            A[k][p] = c * akp - sn * akq; A[k][q] = sn * akp + c * akq;
          }
#pragma unroll
          for (int k = 0; k < D; ++k) {       // A <- J^T A (rows p, q)
            const double apk = A[p][k], aqk = A[q][k];
            A[p][k] = c * apk - sn * aqk; A[q][k] = sn * apk + c * aqk;
          }
#pragma unroll
          for (int k = 0; k < D; ++k) {
            const double vkp = V[k][p], vkq = V[k][q];
            V[k][p] = c * vkp - sn * vkq; V[k][q] = sn * vkp + c * vkq;
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < D; ++k) {
    eig[k] = (T)A[k][k];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      eig[EIG_QT(D) + k * D + i] = (T)V[i][k];
      double tin = 0, tout = 0;                 // Tin[k][i] = sum_j Q[j][k] L[i][j];  Tout[k][i] = sum_j Li[j][k] Q[j][i]
#pragma unroll
      for (int j = 0; j < D; ++j) { tin += V[j][k] * Lm[i][j]; tout += Li[j][k] * V[j][i]; }
      eig[EIG_TIN(D) + k * D + i] = (T)tin;
      eig[EIG_TOUT(D) + k * D + i] = (T)tout;
    }
  }
}

template <typename T, int D, bool DIAG>
__global__ __launch_bounds__(256) void hmc_gauss_eig_kernel(GaussArgs<T> a, const T* __restrict__ eig) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= a.C) return;
  constexpr int NP = D / 2;
  constexpr bool R = (D & 1) != 0;
  T lam[D], Tin[D][D], Tout[D][D], mu[D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    lam[i] = eig[i]; mu[i] = a.mu[i];
#pragma unroll
    for (int k = 0; k < D; ++k) { Tin[i][k] = eig[EIG_TIN(D) + i * D + k]; Tout[i][k] = eig[EIG_TOUT(D) + i * D + k]; }
  }
  const T eps = a.eps, he = (T)0.5 * a.eps;
  T nel[D], hl[D], hlam[D];                      // -eps lam, eps/2 lam, lam/2
#pragma unroll
  for (int i = 0; i < D; ++i) { nel[i] = -(eps * lam[i]); hl[i] = he * lam[i]; hlam[i] = (T)0.5 * lam[i]; }
  const size_t C = (size_t)a.C;
  auto to_y = [&](const T* __restrict__ q, T (&y)[D]) {
    T d[D];
#pragma unroll
    for (int i = 0; i < D; ++i) d[i] = q[i] - mu[i];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      T acc = Tin[k][0] * d[0];
#pragma unroll
      for (int i = 1; i < D; ++i) acc = fma(Tin[k][i], d[i], acc);
      y[k] = acc;
    }
  };
  auto potential = [&](const T (&y)[D]) {          // 0.5 y^T diag(lam) y
    T q = hlam[0] * y[0] * y[0];
#pragma unroll
    for (int i = 1; i < D; ++i) q = fma(hlam[i] * y[i], y[i], q);
    return q;
  };
  T yc[D];
  to_y(a.theta + c * D, yc);
  T quadc = potential(yc);
  int32_t rejected = 0;

  T z[D], logu = 0;
  const T* rec = a.ws_z + (size_t)c * rec_elems<T, D>();
  const size_t rec_step = C * rec_elems<T, D>();
  load_record<T, D>(rec, 0, z, logu);
  // unconditional sample stores, primed once before the loop: see hmc_gauss_small_kernel
  T* const scratch_row = a.theta + c * D;
  T* srow = a.samples ? a.samples + ((size_t)(a.traj_offset > a.burn ? a.traj_offset - a.burn : 1) * C + c) * D
                      : scratch_row;
  const size_t srow_step = a.samples ? C * D : 0;
  // the stored row is kept as it was written: a rejected trajectory repeats the previous row bit for bit (the first rows
  // params_init itself, S:1018); only an accepted proposal is mapped back, q = mu + Tout y
  T qc[D];
#pragma unroll
  for (int i = 0; i < D; ++i) qc[i] = scratch_row[i];
  auto to_q = [&](const T (&y_)[D], T (&q_)[D]) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
      T acc_ = mu[i];
#pragma unroll
      for (int k = 0; k < D; ++k) acc_ = fma(Tout[i][k], y_[k], acc_);
      q_[i] = acc_;
    }
  };
  auto store_q = [&](T* __restrict__ dst) {
#pragma unroll
    for (int i = 0; i < D; ++i) dst[i] = qc[i];
  };
  {                          // the same store a trajectory issues (to rounding the value it overwrites): keeps vmcnt uniform
    T q0[D];
    to_q(yc, q0);
#pragma unroll
    for (int i = 0; i < D; ++i) scratch_row[i] = q0[i];
  }
  for (int t = 0; t < a.n_traj; ++t) {
    const int n = a.traj_offset + t;
    T zn[D], logun = 0;
    rec += rec_step;
    load_record<T, D>(rec, 0, zn, logun);
    // ---- gibbs (S:185-186): r = Q^T z, rotated by the pre-draw pass
    T r[D], y[D];
    T kin = z[0] * z[0];
#pragma unroll
    for (int i = 1; i < D; ++i) kin = fma(z[i], z[i], kin);
    const T h_old = -(a.log_norm - quadc) + (T)0.5 * kin;          // S:971
    // ---- leapfrog (S:973 -> S:281-302)
#pragma unroll
    for (int i = 0; i < D; ++i) { y[i] = yc[i]; r[i] = fma(-hl[i], yc[i], z[i]); }   // S:281
    if constexpr (sizeof(T) == 4 && D >= 2) {
      f2 yP[NP], rP[NP], eP[NP], nP[NP];
      float yS = 0, rS = 0;
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        yP[j] = f2{y[2 * j], y[2 * j + 1]}; rP[j] = f2{r[2 * j], r[2 * j + 1]};
        eP[j] = f2{eps, eps}; nP[j] = f2{nel[2 * j], nel[2 * j + 1]};
      }
      if (R) { yS = y[D - 1]; rS = r[D - 1]; }
      repeat_steps(a.L, [&]() {                                     // S:283-298 (drift, then the merged kick)
#pragma unroll
        for (int j = 0; j < NP; ++j) yP[j] = __builtin_elementwise_fma(eP[j], rP[j], yP[j]);
        if (R) yS = fmaf(eps, rS, yS);
#pragma unroll
        for (int j = 0; j < NP; ++j) rP[j] = __builtin_elementwise_fma(nP[j], yP[j], rP[j]);
        if (R) rS = fmaf(nel[D - 1], yS, rS);
      });
#pragma unroll
      for (int j = 0; j < NP; ++j) { y[2 * j] = yP[j].x; y[2 * j + 1] = yP[j].y; r[2 * j] = rP[j].x; r[2 * j + 1] = rP[j].y; }
      if (R) { y[D - 1] = yS; r[D - 1] = rS; }
    } else {
      repeat_steps(a.L, [&]() {
#pragma unroll
        for (int i = 0; i < D; ++i) y[i] = fma(eps, r[i], y[i]);
#pragma unroll
        for (int i = 0; i < D; ++i) r[i] = fma(nel[i], y[i], r[i]);
      });
    }
#pragma unroll
    for (int i = 0; i < D; ++i) r[i] = fma(hl[i], y[i], r[i]);      // S:302
    const T quad1 = potential(y);
    // ---- H_new (S:995), MH (S:1000-1004)
    const T logp1 = a.log_norm - quad1;
    T kin1 = r[0] * r[0];
#pragma unroll
    for (int i = 1; i < D; ++i) kin1 = fma(r[i], r[i], kin1);
    const T h_new = -logp1 + (T)0.5 * kin1;
    const bool acc = mh_accept_logu<T>(h_old, h_new, logp1, logu);
    // ---- bookkeeping (S:1007-1026; Q2 reset at n == burn+1)
    rejected += acc ? 0 : 1;
    T qp[D];
    to_q(y, qp);
#pragma unroll
    for (int i = 0; i < D; ++i) { yc[i] = acc ? y[i] : yc[i]; qc[i] = acc ? qp[i] : qc[i]; }
    quadc = acc ? quad1 : quadc;
    if (__builtin_expect(n == a.burn + 1, 0)) {                      // wave-uniform, once per run: kept off the hot path
      if (!acc) {
        to_y(a.theta_init + c * D, yc);
        quadc = potential(yc);
#pragma unroll
        for (int i = 0; i < D; ++i) qc[i] = a.theta_init[c * D + i];
      }
    }
    {
      const bool keep = n > a.burn;
      store_q(keep ? srow : scratch_row);
      srow += keep ? srow_step : 0;
    }
    if (DIAG) {
      if (a.H_old) a.H_old[(size_t)t * C + c] = h_old;
      if (a.H_new) a.H_new[(size_t)t * C + c] = h_new;
      if (a.accept) a.accept[(size_t)t * C + c] = acc ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < D; ++j) z[j] = zn[j];
    logu = logun;
  }
  store_q(scratch_row);
  if (a.reject_count) a.reject_count[c] += rejected;
}

template <typename T, int D, int MASS>
__global__ void leapfrog_gauss_small_kernel(GaussArgs<T> a) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= a.C) return;
  SmallModel<T, D, MASS> m;
  m.load(a, false);
  T d[D], p[D], Pd[D];
#pragma unroll
  for (int i = 0; i < D; ++i) { d[i] = a.theta[c * D + i] - m.mu[i]; p[i] = a.p_io[c * D + i]; }
  m.curv_d(d, Pd);
  m.template leapfrog<true>(d, p, Pd, a.L, a.path_theta ? a.path_theta + c * D : nullptr,
                            a.path_p ? a.path_p + c * D : nullptr, a.C * D);
#pragma unroll
  for (int i = 0; i < D; ++i) {
    a.theta[c * D + i] = d[i] + m.mu[i]; a.p_io[c * D + i] = p[i];
    if (a.path_p && a.L > 0) a.path_p[((int64_t)(a.L - 1) * a.C + c) * D + i] = p[i];  // S:302
  }
}

}  // namespace hta
