// Fused HMC for a dense Gaussian target: whole trajectories in one launch, state on-chip.
//
// Replaces, for log p(x) = log_norm - 0.5 (x-mu)^T P (x-mu), the per-trajectory body of
// hamiltorch.sample() (hamiltorch/samplers.py:965-1026):
//   gibbs (S:969 -> S:185-202) -> hamiltonian (S:971 -> S:779-815) -> leapfrog (S:973 -> S:281-302)
//   -> hamiltonian (S:995) -> acceptance + MH test (S:1000-1004) -> burn / store bookkeeping (S:1007-1026)
// for C independent chains.  HBM is touched only at trajectory boundaries (one coalesced [C,D]
// sample row per stored trajectory); theta, p, the gradient and both energies live in registers.
//
// Two layouts:
//   small  (D <= 6):   one chain per lane, D compile-time, P/mu in SGPRs (wave-uniform loads).
//                      This is BASELINE config 2 (3-D, 1024 chains): latency/issue bound, 16 waves.
//   general (D <= 1024): one chain per 64-lane wave, lane l owns elements l, l+64, ...;
//                      P streamed row-by-row (coalesced, L1/L2 resident), the offset vector
//                      broadcast through LDS, energies by wave butterfly reduction.
#include <cstring>
#include <iterator>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>
#include "common.hpp"
#include "philox.hpp"
#include "hmc_gaussian.hpp"
#include "rmhmc.hpp"

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


// =============================================================================================
// D <= 4, fp32, identity mass, latency regime: one chain per DPP quad, one eigen-coordinate per lane
//
// In the eigenbasis the coordinates of a chain do not interact DURING a trajectory, so lane k of a quad integrates
// coordinate k alone: a step is the two dependent FMAs  y += eps r ; r -= eps lam_k y  and nothing else (the chain-per-lane
// kernel above issues four instructions per step at D = 3).  Lanes meet only at trajectory boundaries:
//   * accept test: h_old - h_new = sum_k (0.5 z_k^2 + 0.5 lam_k yc_k^2) - (0.5 r_k^2 + 0.5 lam_k y_k^2)  (log_norm cancels),
//     one two-stage quad butterfly (DPP quad_perm) of the per-lane difference; every lane gets the same decision;
//   * sample row: q_i = mu_i + sum_k Q[i][k] yc_k, lane i broadcasting yc_k from lane k (DPP quad_perm:[k,k,k,k]);
//   * the draw record [Q^T z, log u, pad] is read one element per lane; log u is lane D's element (D < 4).
// A lane >= D of the quad is a dummy coordinate (lam = 0, momentum 0).  1024 chains are 64 waves instead of 16; the
// dispatcher takes this kernel while the chip has idle SIMDs for the extra waves (C <= g_quad_max_chains) and the
// chain-per-lane kernel beyond, where instruction count per chain decides.
// =============================================================================================
#ifndef QUAD_FUSED_NS
#define QUAD_FUSED_NS 4
#endif
// Developer builds only (profiles/r05y_quad_ablation.txt: timing of the trajectory's parts, wrong samples): -DQUAD_FUSED_NS=n -DQUAD_SLOTS=m (a deeper
// record look-ahead: measured, no effect), -DQUAD_ABLATE_STORE / _LOAD / _ACC / _TAIL (one cost of a trajectory removed at a time),
// -DQUAD_ABLATE_ROWS (profiles/r07a_quad_rows.txt: the integrating wave of "quad_rows" with nobody reading its ring), -DQUAD_ABLATE_LOCAL
// (profiles/r08a_quad_local.txt: the local launch whose producer waves draw nothing), -DQUAD_ABLATE_WIDE (below), -DQUAD_ROWS_NI=1|4
// (the other placements of the row waves: correct samples).
#ifndef QUAD_SLOTS
#define QUAD_SLOTS 4
#endif
// -DQUAD_ABLATE_WIDE (profiles/r11a_quad_wide.txt, timing only, wrong samples): the gate of "quad_wide" - in hmc_gauss_quad_local_kernel
// the integrating wave issues its record read and its message write only at position P % 4 == 3 of a group, as one 16-byte access
// each (junk data, lane base x 16 bytes), the other positions pad the wait state with s_nop; barriers untouched, the row wave
// ignores the status message.
#if defined(QUAD_ABLATE_WIDE)
constexpr bool QUAD_ABLATE_WIDE_ON = true;
#else
constexpr bool QUAD_ABLATE_WIDE_ON = false;
#endif
constexpr int QUAD_SLOTS_MAX = QUAD_SLOTS;     // record look-ahead of the quad kernel = rows of slack in the workspace
template <int CTRL> __device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
template <int K> __device__ __forceinline__ float quad_bcast(float v) { return dpp_f<K * 0x55>(v); }
__device__ __forceinline__ float quad_sum(float v) {
  v += dpp_f<0xB1>(v);          // quad_perm:[1,0,3,2]
  v += dpp_f<0x4E>(v);          // quad_perm:[2,3,0,1]
  return v;
}

// LB > 0: a.L == LB is known at compile time (straight-line steps, no loop bookkeeping: at this size every scalar
// instruction on the hot path costs what a vector one does); LB == 0: any L.
//
// VAR (tuning key "quad_variant", default 7) - the same arithmetic, fewer instructions around it (a lone wave pays ~2 ns for
// ANY instruction, so the 28 that are not the trajectory's 52 dependent FMAs are a third of its time):
//   bit 0  addresses as a wave-uniform base (an SGPR pair, advanced once per pass of the unrolled loop) plus a 32-bit lane
//          offset per position of that loop (loop-invariant registers): no 64-bit vector add per record load and per row store
//          (the VAR = 0 loop spends 27 of its 320 instructions per four trajectories on address arithmetic, this one 8);
//   bit 1  no NaN guard in front of the accept compare: the record's 2 log u is finite by construction (u23: 23-bit uniforms
//          in (0, 1)), the energy difference is finite, -inf or NaN (sums of squares cannot reach -inf, the current point is
//          finite), and both -inf >= x and NaN >= x are false - the guard never changes a decision.
//   bit 2  the row element and the quad butterfly of the energy difference as ONE interleaved block (see TAIL below).
// Results are bit-identical to VAR = 0 (tests/test_gpu_hmc.py::test_quad_kernel_variants_are_bit_identical).  Measured at BASELINE
// config 2 (profiles/r03v_*): 166.3 us (VAR 0) -> 157.5 us (VAR 7) per 1000-trajectory launch; the static count 78.5 -> 73.25
// instructions per trajectory (tools/isa_of.py --loops) predicted 155.  With 16 trajectories per pass at L = 25: 72.6, 156.6 us.
template <int I, int N, typename F> __device__ __forceinline__ void quad_static_for(F&& f) {
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); quad_static_for<I + 1, N>(f); }
}
// FUSED (round 4, tuning key "quad_fused"): the pre-draw pass runs INSIDE the same launch - the blocks behind the consumers' are
// producers (quad_fused_kernel below) that write the records chunk by chunk (CH whole trajectories: no 128-byte line straddles two
// chunks) and count themselves into `flags[chunk]` with a release at agent scope; a consumer checks, once per pass of its unrolled
// loop, that the rows the pass prefetches are complete (`ready`: a register compare), polling a chunk's counter only when it
// crosses into that chunk, with the next chunk's counter requested one chunk ahead.  Same records, same arithmetic: results are
// bit-identical to the two-launch form.
// HAND-OVER FAILURE (round 5).  The consumers wait for producers of the SAME grid: that is safe only while both are resident, which
// a launch of 80-320 blocks on an idle 256-CU chip is, and a shared or preempted GPU need not be.  The wait is bounded; a consumer
// whose bound expires does NOT read on (round 4 did: plausible, wrong samples with rc 0): it raises the workspace's STICKY status
// word (`err`: set with an atomic OR, zeroed only by hta_hmc_gaussian_prepare, readable by the host at the byte offset
// hta_hmc_gaussian_status_offset returns), stops waiting, and when its trajectories are done overwrites every row it stored in this
// launch and its slot of the chain state with NaN - the failure is in the data as well as in the word.  All of it is off the hot
// path (inside the once-per-chunk poll and after the loops).  Debug key "quad_starve" makes the producers leave at once (the test
// of this path: tests/test_gpu_hmc.py::test_fused_launch_reports_starved_producers).
// The LOCAL launch (hmc_gauss_quad_local_kernel, tuning key "quad_local", the default for D <= 3 with row waves) has no such hand-over:
// its producers are waves of the consumer's own block, behind a barrier.  It takes none of the fields below; "quad_starve" = 1 - a
// producer BLOCK that is never scheduled - selects this cross-block launch, the only one that failure can happen to.
struct QuadFused { uint32_t* flags; int ch; uint32_t target; int nchunks; uint32_t* err; int starve; };
// ROWS (tuning key "quad_rows", default 1): the OUTPUT side of a chain - the proposal's row element q = mu + Tout y, the select of the
// stored element, the row store, the final state, the reject count, the NaN rows of a starved launch - runs on a ROW WAVE of the
// same workgroup (quad_rows_body below); the integrating wave keeps the chain and the accept test and hands each trajectory's
// outcome over through LDS.
//   message   one dword per trajectory and lane: acc ? y : 0xFFFFFFFF.  The sentinel is a NaN pattern, and an accepted y is never
//             NaN (a NaN or infinite y makes lam y^2, hence dH, NaN or -inf, which the compare rejects; a lane with lam = 0 adds a
//             finite eps r to a finite y), so the row wave rebuilds acc and q exactly: the same v_fmac_f32_dpp sequence on the same y.
//   ring      per integrating wave two buffers of one pass each (NU positions x 64 lanes); the slot address is the lane's base
//             register plus the immediate offset of the position in the unrolled pass - no address arithmetic on the hot path.
//   cost      <3, 25>: 67.5 instructions per trajectory on the integrating wave instead of 73.3 (tests/test_quad_rows_resources.py
//             holds it under 68); 0.148 -> 0.139 ms per 1000 trajectories at BASELINE config 2 (profiles/r07a_quad_rows.txt).
//   hand-over one "s_waitcnt lgkmcnt(0) ; s_barrier" per GROUP of trajectories (a pass of NU, a tail pass of NS, a single one) on
//             both roles: the integrator after it filled buffer g % 2, the row wave before it reads it.  The row wave reaches barrier
//             g + 1 only after it has read group g, and the integrator refills buffer g % 2 only after barrier g + 1.  Both roles
//             derive the sequence of groups from the same launch arguments (quad_groups), so every wave of the block - also one
//             whose chains lie past a.C: it integrates the last chain again and stores nothing - reaches every barrier.
// Results are bit-identical to "quad_rows" = 0 (tests/test_gpu_quad_rows.py).
// LOCAL (hmc_gauss_quad_local_kernel below) is ROWS with the record coming from LDS too: the refill between the two butterfly stages
// is a ds_read_b32 at lane base + immediate, the producer waves join the group's barrier, and there is no need_rows.  <3, 25>: 67.6
// instructions per trajectory, no global memory instruction in the pass (tests/test_quad_local_resources.py).
constexpr int quad_fused_ns(int LB, bool FUSED) { return FUSED ? QUAD_FUSED_NS : (LB == 5 ? 4 : (LB == 10 ? 3 : 2)); }
constexpr int quad_nu(int LB, int NS, bool UADDR) { return UADDR ? (LB == 25 ? (NS > 4 ? 4 : 8) : 4) * NS : 2 * NS; }
constexpr uint32_t QUAD_ROWS_REJECT = 0xFFFFFFFFu;
// The groups of trajectories of a LOCAL launch (hmc_gauss_quad_local_kernel), in order: f(first trajectory, phase, size, Q2).  The
// integrating wave, its row wave and the producer waves all walk THIS sequence, derived from the launch arguments alone, so every
// wave of a block reaches the same barriers.  It is the fused launch's sequence (the Q2 trajectory alone, passes of NU, passes of
// NS, single ones; per phase) with one short group of NS in front: the integrator starts after one producer sweep, not after a pass.
template <int NS, int NU, typename F> __device__ __forceinline__ void quad_local_groups(const GaussArgs<float>& a, F&& f) {
  const int n_burn = a.samples ? min(max(a.burn - a.traj_offset + 1, 0), a.n_traj) : a.n_traj;
  std::integral_constant<int, 1> one;
  std::false_type plain;
  int t = 0;
  for (int phase = 0; phase < 2; ++phase) {
    const int t_end = phase == 0 ? n_burn : a.n_traj;
    if (phase == 1 && t < t_end && a.traj_offset + t == a.burn + 1) { f(t, phase, one, std::true_type{}); t += 1; }
    if (t == 0 && NS - 1 < t_end) { f(t, phase, std::integral_constant<int, NS>{}, plain); t += NS; }
    while (t + NU - 1 < t_end) { f(t, phase, std::integral_constant<int, NU>{}, plain); t += NU; }
    while (t + NS - 1 < t_end) { f(t, phase, std::integral_constant<int, NS>{}, plain); t += NS; }
    while (t < t_end) { f(t, phase, one, plain); t += 1; }
  }
}
// WIDE (hmc_gauss_quad_wide_kernel below, tuning key "quad_wide") is LOCAL with 16-byte hand-overs: both rings keep their sizes, but
// position p WITHIN ITS GROUP lives at (p >> 2) * 1024 + lane * 16 + (p & 3) * 4 of a buffer (lane: the integrating wave's), so the
// four positions of a block of four are one ds_read_b128 / ds_write_b128 per lane.  The integrating wave reads the records of block
// b + 1 inside the first trajectory of block b into the other half of eight record registers (one wait per block) and writes the
// four messages of a block with the select that completes it (or in the hand-over); the butterfly's wait states that were LDS
// instructions are one "s_nop 1".  The 16-byte accesses are typed LDS accesses the compiler sees: it keeps their wait counts and
// the hazard of a wide store's data registers.  Arithmetic, the sequence of groups (quad_local_groups) and the number and order of
// s_barriers of every role are exactly LOCAL's - only addresses and LDS instructions differ, so there is no new way to hang.
template <int D, bool DIAG, int LB, int VAR, bool FUSED, bool ROWS = false, bool LOCAL = false, bool WIDE = false>
__device__ __forceinline__ void quad_body(const GaussArgs<float>& a, const float* __restrict__ eig, const int64_t gt, const QuadFused fz,
                                          uint32_t lds = 0, uint32_t recl = 0) {
  typedef float T;
  constexpr bool UADDR = (VAR & 1) != 0, NOGUARD = (VAR & 2) != 0, TAIL = (VAR & 4) != 0;
  static_assert(!ROWS || (FUSED && UADDR && TAIL && !DIAG), "the row-wave form is an instance of the fused launch");
  static_assert(!LOCAL || (ROWS && D < 4), "the local launch is the row-wave form with one record vector");
  static_assert(!WIDE || (LOCAL && QUAD_FUSED_NS == 4), "the wide hand-over is the local launch's, in blocks of four positions");
  typedef float V4f __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) V4f* lvec_t;
  const bool on = (gt >> 2) < a.C;
  const int64_t c = ROWS ? (on ? gt >> 2 : a.C - 1) : gt >> 2;       // ROWS: every wave stays for the barriers
  const int k = (int)(gt & 3);
  if constexpr (!ROWS) { if (c >= a.C) return; }                     // whole quads leave together
  // FUSED: rows [0, ready) are known complete; the counter of the chunk that starts at row `ready` was requested when the previous
  // chunk was confirmed (pf).  The hot path pays one compare per pass; the poll runs once per chunk, out of the straight line.
  int ready = 0;
  uint32_t pf = 0;
  bool starved = false;
  if constexpr (FUSED && !LOCAL) pf = __hip_atomic_load(fz.flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  auto need_rows = [&](int upto) {              // rows up to `upto` are about to be read (rows >= n_traj are slack: never produced)
    if constexpr (FUSED && !LOCAL) {            // (LOCAL: the block's own producer waves, published by the barrier of the group)
      if (__builtin_expect(upto >= ready, 0)) {
        do {
          const int chn = ready / fz.ch;
          if (chn >= fz.nchunks) { ready = 0x7fffffff; break; }
          uint32_t v = pf;
          // (bounded - ~1 s of polling: producers wait for nothing, so they count as soon as they are scheduled; one that is not
          //  would otherwise hang the queue)
          for (int spin = 0; v < fz.target && spin < (1 << 20); ++spin) {
            __builtin_amdgcn_s_sleep(4);
            v = __hip_atomic_load(fz.flags + chn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          if (__builtin_expect(v < fz.target, 0)) {          // the bound expired: sticky status word, no more waiting, NaN rows at the end
            __hip_atomic_fetch_or(fz.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            starved = true;
            ready = 0x7fffffff;
            break;
          }
          ready += fz.ch;
          pf = chn + 1 < fz.nchunks ? __hip_atomic_load(fz.flags + chn + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        } while (upto >= ready);
        __atomic_signal_fence(__ATOMIC_SEQ_CST);  // the record loads below stay below
      }
    }
  };
  const bool live = k < D;
  const int kk = live ? k : 0;                  // a dummy lane (k >= D) mirrors lane 0 on the output side (same address, same value)
  const T lam = live ? eig[kk] : 0.f;
  const T mu = a.mu[kk];
  T Qrow[D], Qcol[D];                           // Q[k][j] and Q[j][k]
#pragma unroll
  for (int j = 0; j < D; ++j) {
    Qrow[j] = eig[EIG_TOUT(D) + kk * D + j];                  // q_k = mu_k + sum_j Tout[k][j] y_j
    Qcol[j] = live ? eig[EIG_TIN(D) + kk * D + j] : 0.f;     // y_k = sum_i Tin[k][i] (q_i - mu_i)
  }
  // a dummy lane integrates nothing: eps = lam = 0, so its y stays 0, its r stays whatever its record slot held (log u or
  // padding) and its energy difference is exactly 0
  const T eps = live ? a.eps : 0.f, nel = -(eps * lam), hl = 0.5f * eps * lam;
  const size_t C = (size_t)a.C;
  auto bc = [&](T v, int j) {                   // lane j of the quad (j compile-time after unrolling)
    return j == 0 ? quad_bcast<0>(v) : j == 1 ? quad_bcast<1>(v) : j == 2 ? quad_bcast<2>(v) : quad_bcast<3>(v);
  };
  auto to_y = [&](const T* __restrict__ q) {    // y_k = sum_i Q[i][k] (q_i - mu_i)
    const T d = live ? q[c * D + kk] - mu : 0.f;
    T y = Qcol[0] * bc(d, 0);
#pragma unroll
    for (int i = 1; i < D; ++i) y = fmaf(Qcol[i], bc(d, i), y);
    return y;
  };
  auto to_q = [&](T y) {                         // q_k = mu_k + sum_j Q[k][j] y_j: v_fmac_f32 with a DPP-broadcast operand
    T q = mu;
    // VALU write of y -> DPP read: 2 wait states (inline asm is not tracked); tied to y so it cannot move ahead of y's producer
    asm volatile("s_nop 1" : "+v"(y));
#pragma unroll
    for (int j = 0; j < D; ++j)
      asm volatile("v_fmac_f32_dpp %0, %1, %2 quad_perm:[%3,%3,%3,%3] row_mask:0xf bank_mask:0xf"
                   : "+v"(q) : "v"(y), "v"(Qrow[j]), "n"(j));
    return q;
  };
  T yc = to_y(a.theta);
  // the row element this lane stores: kept as it was written (a rejected trajectory repeats the previous row bit for bit,
  // the first rows repeat params_init exactly, S:1018) - only an accepted proposal is mapped back, q = mu + Tout y
  T qc = ROWS ? 0.f : a.theta[c * D + kk];        // (ROWS: the row wave's)
  // Energies are carried DOUBLED (2 x potential share = lam y^2, 2 x kinetic share = r^2; the record holds 2 log u): one
  // multiply less per energy, and scaling by two commutes with rounding, so the decisions are those of the plain form.
  T potc = lam * yc * yc;                        // twice this coordinate's share of the potential at the current point
  int32_t accepted = 0;

  // The record pointer is per lane and advances with one 64-bit vector add per trajectory (a scalar base would take an
  // s_add / s_addc pair: at this size a scalar instruction costs what a vector one does).
  constexpr int W = rec_elems<T, D>();
  typedef const __attribute__((address_space(1))) T* grec_t;       // stays a global pointer through the ordering asm below
  grec_t rec = (grec_t)(a.ws_z + (size_t)c * W + k);               // element k of this chain's record (W >= 4 floats)
  const int ushift = D - k;                                        // D == 4: log u sits in the second vector
  const size_t rec_step = C * W;
  // Records are read NS trajectories ahead: a trajectory (~90 ns at L = 5, ~180 ns at L = 25) is shorter than the ~250 ns
  // an HBM load takes to return, and the look-ahead has to cover it.  The workspace carries QUAD_SLOTS_MAX rows of slack.
  constexpr int NS = quad_fused_ns(LB, FUSED);     // (FUSED: the records come from memory, not from this XCD's L2)
  static_assert(NS <= QUAD_SLOTS_MAX, "workspace slack");
  constexpr int NZ = WIDE ? 8 : NS;                // (WIDE: the block being consumed and the block being read)
  T zs[NZ], lus[NZ];
  T mq[4] = {0.f, 0.f, 0.f, 0.f};                  // WIDE: the messages of the block being completed
#if defined(QUAD_ABLATE_WIDE)
  const V4f wzero = {0.f, 0.f, 0.f, 0.f};
  V4f wjunk = wzero;
#endif
  need_rows(NS - 1);
  if constexpr (LOCAL) {
#pragma unroll
    for (int i = 0; i < NZ; ++i) zs[i] = lus[i] = 0.f;      // (begin() below reads the first records of every group)
  } else {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      if (i) rec += rec_step;
      zs[i] = *rec;
      lus[i] = D == 4 ? *(rec + ushift) : 0.f;
    }
  }
  // Every lane stores once per trajectory, unconditionally (uniform vmcnt, see hmc_gauss_small_kernel).
  const uint32_t qoff = (uint32_t)(((size_t)c * D + kk) * sizeof(T));
  typedef __attribute__((address_space(1))) char* gwbytes_t;
  auto put = [&](gwbytes_t row, T v) { *(__attribute__((address_space(1))) T*)(row + qoff) = v; };
  if constexpr (!ROWS) put((gwbytes_t)a.theta, to_q(yc));
  // UADDR: the record of the trajectory at position i of the unrolled loop is recb + roff[i] (recb: the row NS ahead of the
  // pass's first trajectory), its stored row element rowb + soff[i]; both bases are wave-uniform and move once per pass.
  // (the dispatcher bounds C so that the offsets stay below 2^32)
  constexpr int NU = quad_nu(LB, NS, UADDR);       // trajectories per pass of the unrolled loop (the scalar bookkeeping of a pass is shared)
  // ROWS: the message of the trajectory at position i of a group goes to lds + 256 i (64 lanes x 4 bytes); `lds` flips between the two buffers
  const uint32_t lds_both = 2u * lds + (uint32_t)(NU * 256), recl_both = 2u * recl + (uint32_t)(NU * 256);
  T pend_y = 0.f;                                // the last trajectory's proposal and decision: its message is still to be written (D < 4)
  uint64_t pend_mask = 0;
  auto handover = [&](auto G) {                  // after a group of G trajectories
    if constexpr (ROWS) {
      if constexpr (WIDE && decltype(G)::value >= 4) {      // the group's last message completes its last block
        asm volatile("v_cndmask_b32_e64 %0, -1, %1, %2" : "=v"(mq[3]) : "v"(pend_y), "s"(pend_mask));
        *(lvec_t)(uintptr_t)(lds + (uint32_t)((decltype(G)::value / 4 - 1) * 1024)) = V4f{mq[0], mq[1], mq[2], mq[3]};
      } else if constexpr (D < 4) {                          // (WIDE: a group of one is slot 0 of block 0 - the same dword)
        T msg;
        asm volatile("v_cndmask_b32_e64 %0, -1, %1, %2\n\tds_write_b32 %3, %0 offset:%4"
                     : "=&v"(msg) : "v"(pend_y), "s"(pend_mask), "v"(lds), "n"(QUAD_ABLATE_WIDE_ON && LOCAL ? ((decltype(G)::value - 1) >> 2) * 1024 : (decltype(G)::value - 1) * 256));
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      lds = lds_both - lds;
      if constexpr (LOCAL) recl = recl_both - recl;
    }
  };
  // LOCAL: the record element of the trajectory at position i of a group is at recl + 256 i (16 chains x 16 bytes: this lane's element
  // of its chain's record is the lane's own dword), in the buffer the producer waves filled during the previous group and the
  // barrier in front of this one published.  A group reads its first NS elements here and, inside trajectory P, the element of
  // trajectory P + NS - never past the group: the other buffer is being written.
  typedef const __attribute__((address_space(3))) T* lrec_t;
  auto begin = [&](auto G) {
    if constexpr (WIDE && decltype(G)::value >= 4) {      // block 0 of the group; block b + 1 is read inside the first trajectory of block b
      const V4f v = *(lvec_t)(uintptr_t)recl;
      zs[0] = v[0]; zs[1] = v[1]; zs[2] = v[2]; zs[3] = v[3];
    } else if constexpr (LOCAL) {                           // (WIDE: a group of one is slot 0 of block 0 - the same dword)
#pragma unroll
      for (int i = 0; i < (decltype(G)::value < NS ? decltype(G)::value : NS); ++i)      // (volatile: four ds_read_b32, not two paired reads - the loop's count is pinned)
        zs[i] = *(const volatile __attribute__((address_space(3))) T*)(uintptr_t)(recl + (uint32_t)i * 256u);
    }
  };
  typedef const __attribute__((address_space(1))) char* gcbytes_t;
  gcbytes_t recb = (gcbytes_t)a.ws_z + (size_t)NS * (rec_step * sizeof(T));
  uint32_t roff[NU], uoff[NU], soff[NU];
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    roff[i] = (uint32_t)((c * W + k) * sizeof(T)) + (uint32_t)i * (uint32_t)(rec_step * sizeof(T));
    uoff[i] = roff[i] + (uint32_t)(ushift * sizeof(T));
    soff[i] = qoff;
  }
  // Two phases, one loop body: trajectories with n <= burn rewrite the chain's slot of `theta` (row step 0), the others
  // walk the sample rows.
  const int n_burn = a.samples ? min(max(a.burn - a.traj_offset + 1, 0), a.n_traj) : a.n_traj;
  int t = 0;
  for (int phase = 0; phase < 2; ++phase) {
    const int t_end = phase == 0 ? n_burn : a.n_traj;
    gwbytes_t row = (gwbytes_t)a.theta;
    size_t row_step = 0;
    if (phase == 1) {
      row = (gwbytes_t)(a.samples + (size_t)max(a.traj_offset + t - a.burn, 1) * C * D);
      row_step = C * D * sizeof(T);
    }
    if constexpr (UADDR) {
#pragma unroll
      for (int i = 0; i < NU; ++i) soff[i] = qoff + (uint32_t)i * (uint32_t)row_step;
    }
    // one trajectory; `slot` holds its record element and is refilled with the one two trajectories ahead (the loop is
    // unrolled by two over the slots, so the newest load is never touched by a register rotation)
    // `q2`: this is trajectory burn+1, the one the reference resets to params_init when it is rejected (S:1016-1018);
    // a separate instance, so that the others carry no check for it.
    auto trajectory = [&](T& slot, T& slot_u, auto q2, auto pos, auto grp) {      // (grp: the size of the trajectory's group, LOCAL reads it)
      if constexpr (!UADDR) rec += rec_step;
      // everything that reads the record first, so that its register is free for the refill
      // ---- gibbs S:185-186 (rotated draws), H_old S:971, half kick S:281
      T y = yc, r, eo, logu;
      {
        const T z = slot;
        if constexpr (ROWS && D < 4) logu = 0.f;      // (broadcast inside the butterfly block below: one of its wait states)
        else
        logu = D == 4 ? slot_u
                      : __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, z), (D < 4 ? D : 0) * 0x55,
                                                                            0xF, 0xF, true));
        eo = fmaf(z, z, potc);
        r = fmaf(-hl, yc, z);
      }
      // (the empty asm orders the refill after the record's last use, so the load can target the record's own register;
      //  otherwise the scheduler hoists the load and the back-edge copy of its result waits for it)
      if constexpr (ROWS && D < 4) {
      } else if constexpr (UADDR) {
        asm volatile("" : "+v"(roff[pos]) : "v"(r), "v"(eo), "v"(logu));
#if defined(QUAD_ABLATE_LOAD4)      // timing only (needs -DQUAD_FUSED_NS=8 -DQUAD_SLOTS=8): ONE 16-byte load per four trajectories into the four slots just consumed
        if constexpr (decltype(pos)::value % 4 == 3 && NS == 8) {
          typedef float V4f __attribute__((ext_vector_type(4)));
          const V4f q4 = *(const __attribute__((address_space(1))) V4f*)(recb + roff[pos]);
          constexpr int b0 = (decltype(pos)::value % 8) - 3;
          zs[b0] = q4[0]; zs[b0 + 1] = q4[1]; zs[b0 + 2] = q4[2]; zs[b0 + 3] = q4[3];
        }
#elif !defined(QUAD_ABLATE_LOAD)
        slot = *(grec_t)(recb + roff[pos]);
#endif
        if (D == 4) slot_u = *(grec_t)(recb + uoff[pos]);
      } else {
        asm volatile("" : "+v"(rec) : "v"(r), "v"(eo), "v"(logu));
        slot = *rec;
        if (D == 4) slot_u = *(rec + ushift);
      }
      if constexpr (LB > 0) {                                                       // S:283-298
#pragma unroll
        for (int l = 0; l < LB; ++l) { y = fmaf(eps, r, y); r = fmaf(nel, y, r); }
      } else {
        repeat_steps(a.L, [&]() { y = fmaf(eps, r, y); r = fmaf(nel, y, r); });
      }
      r = fmaf(hl, y, r);                                                           // S:302
      // ---- H_new S:995 and the MH test S:1000-1004
      const T pot1 = lam * y * y;
      const T en = fmaf(r, r, pot1);
      // the proposal's row element q_k = mu_k + sum_j Tout[k][j] y_j: v_fmac_f32 with a DPP-broadcast operand.  Ordered after
      // `en` (dummy operand): the instructions since the last write of y are the wait states its DPP read needs.
      T qp, dH;
      static_assert(D >= 1 && D <= 4, "quad kernel");
#define HTA_QF(J, OP) "\n\tv_fmac_f32_dpp %0, %1, %" #OP " quad_perm:[" #J "," #J "," #J "," #J "] row_mask:0xf bank_mask:0xf"
      if constexpr (TAIL) {
        // One block for the row element AND the quad butterfly of the energy difference, interleaved so that every DPP read of
        // a freshly written register has its two wait states from useful instructions (the compiler does not look into inline
        // assembly and pads its own DPP pairs with s_nop: one issue slot per trajectory):
        //   d = eo - en (compiler) | mov qp, mu | qp += Q[k][0] y_0 | d += d[lane^1] | qp += Q[k][1] y_1 | ... | d += d[lane^2]
#define HTA_QG(J, OP) "\n\tv_fmac_f32_dpp %0, %2, %" #OP " quad_perm:[" #J "," #J "," #J "," #J "] row_mask:0xf bank_mask:0xf"
#define HTA_B1 "\n\tv_add_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1"
#define HTA_B2 "\n\tv_add_f32_dpp %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1"
        dH = eo - en;
        if constexpr (ROWS && D < 4) {
          // The row element is the row wave's.  The two wait states in front of each stage of the butterfly are useful instructions:
          //   d = eo - en (compiler) | select of the PREVIOUS trajectory's message | log u broadcast | d += d[lane^1] | LDS write of that
          //   message | record refill (compiler; volatile asm on both sides keeps it there) | d += d[lane^2]
          // - the message of a trajectory is selected and written one trajectory late (the last one of a group: flush, before the
          // hand-over), so the integrating wave spends no s_nop on the butterfly; the first trajectory of a group has no message to
          // carry and pads with two.
          qp = 0.f;
          constexpr int P = decltype(pos)::value;
          if constexpr (WIDE) {
            // The same blocks with the LDS instructions once per block of four positions: the select of trajectory P - 1's message
            // targets mq[(P - 1) % 4]; the select of a block's last message (P % 4 == 0, P > 0) is followed by the 16-byte write of
            // the block, and the first trajectory of a block reads the records of the next block of the group into the other half
            // of zs.  A trajectory that issues no LDS instruction (three of four) has its tail in ONE asm block, the second stage's
            // two wait states being one "s_nop 1" (the compiler pads between two blocks).  The first trajectory of a block keeps
            // the local launch's form: the typed LDS accesses (or an "s_nop 0") sit between two volatile asm blocks and are the
            // wait states of the second stage; tests/test_quad_wide_resources.py checks in the built code that every second
            // stage has its two wait states.
            constexpr int Gs = decltype(grp)::value;
            constexpr bool rd = P % 4 == 0 && P + 4 < Gs, wr = P % 4 == 0 && P > 0;
#define HTA_WB1 "\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1"
#define HTA_WT2 "\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_cmp_ge_f32_e64 %3, %0, %1" \
                "\n\tv_cndmask_b32_e64 %2, %2, %5, %3"
            if constexpr (!rd && !wr && P > 0) {
              asm volatile("v_cndmask_b32_e64 %4, -1, %7, %3\n\tv_mov_b32_dpp %1, %6 quad_perm:[%8,%8,%8,%8] row_mask:0xf bank_mask:0xf bound_ctrl:1"
                           HTA_WB1 "\n\ts_nop 1" HTA_WT2
                           : "+v"(dH), "=&v"(logu), "+v"(yc), "+s"(pend_mask), "=&v"(mq[(P + 3) % 4])
                           : "v"(y), "v"(slot), "v"(pend_y), "n"(D));
            } else if constexpr (!rd && !wr) {
              T none;
              asm volatile("v_mov_b32_dpp %1, %6 quad_perm:[%8,%8,%8,%8] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 0"
                           HTA_WB1 "\n\ts_nop 1" HTA_WT2
                           : "+v"(dH), "=&v"(logu), "+v"(yc), "+s"(pend_mask), "=&v"(none)
                           : "v"(y), "v"(slot), "v"(pend_y), "n"(D));
            } else {
              if constexpr (wr) {
                asm volatile("v_cndmask_b32_e64 %2, -1, %4, %5\n\tv_mov_b32_dpp %1, %3 quad_perm:[%6,%6,%6,%6] row_mask:0xf bank_mask:0xf bound_ctrl:1"
                             HTA_WB1
                             : "+v"(dH), "=&v"(logu), "=&v"(mq[3]) : "v"(slot), "v"(pend_y), "s"(pend_mask), "n"(D));
                *(lvec_t)(uintptr_t)(lds + (uint32_t)((P / 4 - 1) * 1024)) = V4f{mq[0], mq[1], mq[2], mq[3]};
              } else {
                asm volatile("v_mov_b32_dpp %1, %2 quad_perm:[%3,%3,%3,%3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 0" HTA_WB1 "\n\ts_nop 0"
                             : "+v"(dH), "=&v"(logu) : "v"(slot), "n"(D));
              }
              if constexpr (rd) {
                constexpr int nb = P / 4 + 1;
                const V4f v = *(lvec_t)(uintptr_t)(recl + (uint32_t)(nb * 1024));
                zs[(nb % 2) * 4] = v[0]; zs[(nb % 2) * 4 + 1] = v[1]; zs[(nb % 2) * 4 + 2] = v[2]; zs[(nb % 2) * 4 + 3] = v[3];
              } else asm volatile("s_nop 0");
              asm volatile("v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_cmp_ge_f32_e64 %2, %0, %3\n\t"
                           "v_cndmask_b32_e64 %1, %1, %4, %2"
                           : "+v"(dH), "+v"(yc), "=&s"(pend_mask) : "v"(logu), "v"(y));
            }
            // (the select of potc is a block of its own, free to sink to potc's next use; the compiler pads one wait state between
            //  the block above and the next trajectory's first FMA, which reads yc - where the local launch has its s_waitcnt)
            asm volatile("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(potc) : "v"(pot1), "s"(pend_mask));
#undef HTA_WB1
#undef HTA_WT2
            pend_y = y;
          } else {
#if defined(QUAD_ABLATE_WIDE)      // timing only (profiles/r11a_quad_wide.txt): the message write once per four positions as ONE 16-byte write of junk, the others pad
          if constexpr (LOCAL && P > 0) {
            T msg;
            if constexpr (P % 4 == 3)
              asm volatile("v_cndmask_b32_e64 %2, -1, %4, %5\n\tv_mov_b32_dpp %1, %3 quad_perm:[%8,%8,%8,%8] row_mask:0xf bank_mask:0xf bound_ctrl:1"
                           "\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1"
                           "\n\tds_write_b128 %6, %9 offset:%7"
                           : "+v"(dH), "=&v"(logu), "=&v"(msg)
                           : "v"(slot), "v"(pend_y), "s"(pend_mask), "v"(lds), "n"((P >> 2) * 1024), "n"(D), "v"(wzero));
            else
              asm volatile("v_cndmask_b32_e64 %2, -1, %4, %5\n\tv_mov_b32_dpp %1, %3 quad_perm:[%6,%6,%6,%6] row_mask:0xf bank_mask:0xf bound_ctrl:1"
                           "\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1"
                           "\n\ts_nop 0"
                           : "+v"(dH), "=&v"(logu), "=&v"(msg)
                           : "v"(slot), "v"(pend_y), "s"(pend_mask), "n"(D));
          } else
#endif
          if constexpr (P > 0) {
            T msg;
            asm volatile("v_cndmask_b32_e64 %2, -1, %4, %5\n\tv_mov_b32_dpp %1, %3 quad_perm:[%8,%8,%8,%8] row_mask:0xf bank_mask:0xf bound_ctrl:1"
                         "\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1"
                         "\n\tds_write_b32 %6, %2 offset:%7"
                         : "+v"(dH), "=&v"(logu), "=&v"(msg)
                         : "v"(slot), "v"(pend_y), "s"(pend_mask), "v"(lds), "n"((P - 1) * 256), "n"(D));
          } else {
            asm volatile("v_mov_b32_dpp %1, %2 quad_perm:[%3,%3,%3,%3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 0" "\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1" "\n\ts_nop 0"
                         : "+v"(dH), "=&v"(logu) : "v"(slot), "n"(D));
          }
          if constexpr (LOCAL) {
            // the refill is an LDS read the compiler sees and waits for (the message writes it does not see only make its count
            // stricter: LDS returns in order); the last NS trajectories of a group have nothing to read and pad the wait state
#if defined(QUAD_ABLATE_WIDE)      // timing only: ONE 16-byte read per four positions, waited for four trajectories later (nobody uses it: the slots keep begin()'s records)
            if constexpr (P % 4 == 3 && P + NS < decltype(grp)::value) {
              asm volatile("" :: "v"(wjunk));
              wjunk = *(lvec_t)(uintptr_t)(recl + (uint32_t)(((P + 1) >> 2) * 1024));
            }
            else asm volatile("s_nop 0");
#else
            if constexpr (P + NS < decltype(grp)::value) slot = *(lrec_t)(uintptr_t)(recl + (uint32_t)(P + NS) * 256u);
            else asm volatile("s_nop 0");
#endif
          } else {
          asm volatile("" : "+v"(roff[pos]));            // keeps the zero-extension next to its use: base + 32-bit offset addressing
          slot = *(grec_t)(recb + roff[pos]);
          }
          // second stage, the compare and the selects of yc and potc in one block (the compiler pads a wait state between two blocks)
          asm volatile("v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_cmp_ge_f32_e64 %3, %0, %4\n\t"
                       "v_cndmask_b32_e64 %1, %1, %5, %3\n\tv_cndmask_b32_e64 %2, %2, %6, %3"
                       : "+v"(dH), "+v"(yc), "+v"(potc), "=&s"(pend_mask) : "v"(logu), "v"(y), "v"(pot1));
          pend_y = y;                                    // its message: inside the next trajectory's block, or by the hand-over
          }
        }
        else if constexpr (ROWS) { qp = 0.f; dH = quad_sum(dH); }      // (D = 4: log u is a second record element; the compiler pads the DPP wait states)
        else if constexpr (D == 1)
          asm volatile("v_mov_b32 %0, %3" HTA_QG(0, 4) HTA_B1 "\n\ts_nop 1" HTA_B2
                       : "=&v"(qp), "+v"(dH) : "v"(y), "v"(mu), "v"(Qrow[0]));
        else if constexpr (D == 2)
          asm volatile("v_mov_b32 %0, %3" HTA_QG(0, 4) HTA_B1 HTA_QG(1, 5) "\n\ts_nop 0" HTA_B2
                       : "=&v"(qp), "+v"(dH) : "v"(y), "v"(mu), "v"(Qrow[0]), "v"(Qrow[D > 1 ? 1 : 0]));
#if defined(QUAD_ABLATE_TAIL)
        else if constexpr (D == 3) qp = y;
#endif
        else if constexpr (D == 3)
          asm volatile("v_mov_b32 %0, %3" HTA_QG(0, 4) HTA_B1 HTA_QG(1, 5) HTA_QG(2, 6) HTA_B2
                       : "=&v"(qp), "+v"(dH) : "v"(y), "v"(mu), "v"(Qrow[0]), "v"(Qrow[D > 1 ? 1 : 0]), "v"(Qrow[D > 2 ? 2 : 0]));
        else
          asm volatile("v_mov_b32 %0, %3" HTA_QG(0, 4) HTA_B1 HTA_QG(1, 5) HTA_QG(2, 6) HTA_B2 HTA_QG(3, 7)
                       : "=&v"(qp), "+v"(dH) : "v"(y), "v"(mu), "v"(Qrow[0]), "v"(Qrow[D > 1 ? 1 : 0]), "v"(Qrow[D > 2 ? 2 : 0]),
                         "v"(Qrow[D > 3 ? 3 : 0]));
#undef HTA_QG
#undef HTA_B1
#undef HTA_B2
      } else {
        if constexpr (D == 1)
          asm volatile("v_mov_b32 %0, %2" HTA_QF(0, 4) : "=&v"(qp) : "v"(y), "v"(mu), "v"(en), "v"(Qrow[0]));
        else if constexpr (D == 2)
          asm volatile("v_mov_b32 %0, %2" HTA_QF(0, 4) HTA_QF(1, 5)
                       : "=&v"(qp) : "v"(y), "v"(mu), "v"(en), "v"(Qrow[0]), "v"(Qrow[D > 1 ? 1 : 0]));
        else if constexpr (D == 3)
          asm volatile("v_mov_b32 %0, %2" HTA_QF(0, 4) HTA_QF(1, 5) HTA_QF(2, 6)
                       : "=&v"(qp) : "v"(y), "v"(mu), "v"(en), "v"(Qrow[0]), "v"(Qrow[D > 1 ? 1 : 0]), "v"(Qrow[D > 2 ? 2 : 0]));
        else
          asm volatile("v_mov_b32 %0, %2" HTA_QF(0, 4) HTA_QF(1, 5) HTA_QF(2, 6) HTA_QF(3, 7)
                       : "=&v"(qp) : "v"(y), "v"(mu), "v"(en), "v"(Qrow[0]), "v"(Qrow[D > 1 ? 1 : 0]), "v"(Qrow[D > 2 ? 2 : 0]),
                         "v"(Qrow[D > 3 ? 3 : 0]));
        dH = quad_sum(eo - en);                                                       // 2 (h_old - h_new)
      }
#undef HTA_QF
      // the decision as a lane mask (v_cmp into an SGPR pair), consumed by a carry-in add and two selects
      // rho = min(0, dH) >= log u  <=>  dH >= log u, because log u <= 0 (S:1000-1004).  A non-finite dH must reject:
      // fma(dH, 0, dH) is dH when dH is finite and NaN otherwise (inf * 0), and NaN >= x is false - one compare in all.
#if defined(QUAD_ABLATE_ACC)
      const uint64_t accmask = ~0ull; asm volatile("" :: "v"(dH), "v"(logu));
#else
      const uint64_t accmask = (ROWS && D < 4) ? pend_mask : __builtin_amdgcn_fcmpf(NOGUARD ? dH : __builtin_fmaf(dH, 0.0f, dH), logu, 3 /* oge */);
#endif
      if constexpr (ROWS) {
        // yc, potc <- accepted point; the message acc ? y : sentinel (-1 is an inline constant) into this position's slot of the ring.
        // The accepted count is the row wave's as well.  (D < 4: all of it happened in the butterfly blocks above.)
        if constexpr (D == 4) {
          T msg;
          asm volatile("v_cndmask_b32_e64 %0, %0, %3, %5\n\tv_cndmask_b32_e64 %1, %1, %4, %5\n\tv_cndmask_b32_e64 %2, -1, %3, %5\n\t"
                       "ds_write_b32 %6, %2 offset:%7"
                       : "+v"(yc), "+v"(potc), "=&v"(msg)
                       : "v"(y), "v"(pot1), "s"(accmask), "v"(lds), "n"(decltype(pos)::value * 256));
        }
        if constexpr (decltype(q2)::value) {
          if (!((accmask >> (threadIdx.x & 63)) & 1)) { yc = to_y(a.theta_init); potc = lam * yc * yc; }      // Q2: back to params_init itself
        }
      } else if constexpr (!decltype(q2)::value) {
        // accepted += acc; yc, potc, qc <- accepted point: a carry-in add and three selects on the accept mask
        uint64_t carry_out;
        asm volatile("v_addc_co_u32_e64 %0, %4, 0, %0, %5\n\tv_cndmask_b32_e64 %1, %1, %6, %5\n\tv_cndmask_b32_e64 %2, %2, %7, %5\n\t"
                     "v_cndmask_b32_e64 %3, %3, %8, %5"
                     : "+v"(accepted), "+v"(yc), "+v"(potc), "+v"(qc), "=&s"(carry_out)
                     : "s"(accmask), "v"(y), "v"(pot1), "v"(qp));
      } else {
        uint64_t carry_out;
        asm("v_addc_co_u32_e64 %0, %1, 0, %0, %2" : "+v"(accepted), "=s"(carry_out) : "s"(accmask));
        asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(yc) : "v"(y), "s"(accmask));
        asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(potc) : "v"(pot1), "s"(accmask));
        asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(qc) : "v"(qp), "s"(accmask));
        if (!((accmask >> (threadIdx.x & 63)) & 1)) {        // Q2: back to params_init itself
          yc = to_y(a.theta_init); potc = lam * yc * yc; qc = a.theta_init[c * D + kk];
        }
      }
      if constexpr (ROWS) {
      } else if constexpr (UADDR) {
        asm volatile("" : "+v"(soff[pos]));            // keeps the zero-extension next to its use: base + 32-bit offset addressing
#if !defined(QUAD_ABLATE_STORE)
        *(__attribute__((address_space(1))) T*)(row + soff[pos]) = qc;
#endif
      } else {
        put(row, qc);
        row += row_step;
      }
      if (DIAG) {
        const bool acc = (accmask >> (threadIdx.x & 63)) & 1;
        // (a dummy lane's eo and en are both the square of its record slot - 2 log u on lane D: they cancel in dH, not in the energies)
        const T ho = 0.5f * quad_sum(live ? eo : 0.f) - a.log_norm, hn = 0.5f * quad_sum(live ? en : 0.f) - a.log_norm;
        if (k == 0) {
          if (a.H_old) a.H_old[(size_t)t * C + c] = ho;
          if (a.H_new) a.H_new[(size_t)t * C + c] = hn;
          if (a.accept) a.accept[(size_t)t * C + c] = acc ? 1 : 0;
        }
      }
      ++t;
    };
    std::false_type plain;
    std::integral_constant<int, 0> first;
    auto rotate = [&]() {                       // slot 0 was consumed and refilled with the newest row: it becomes the last
      const T z = zs[0], u = lus[0];
#pragma unroll
      for (int i = 0; i + 1 < NS; ++i) { zs[i] = zs[i + 1]; lus[i] = lus[i + 1]; }
      zs[NS - 1] = z; lus[NS - 1] = u;
    };
    if constexpr (LOCAL) {
      // the groups of the launch as every role of the block walks them (quad_local_groups); the barrier in front of the first
      // group publishes its records
      if (phase == 0) {
        asm volatile("s_barrier" ::: "memory");
        quad_local_groups<NS, NU>(a, [&](int, int, auto G, auto q2) {
          begin(G);
          quad_static_for<0, decltype(G)::value>([&](auto I) { trajectory(zs[I % NZ], lus[I % NZ], q2, I, G); });
          handover(G);
        });
      }
    } else if constexpr (UADDR) {
      // the same schedule with the bases moved once per group of trajectories
      auto moved = [&](int g) { recb += (size_t)g * (rec_step * sizeof(T)); row += (size_t)g * row_step; };
      // (FUSED: a pass of G trajectories starting at t prefetches the rows up to t + G - 1 + NS)
      if (phase == 1 && t < t_end && a.traj_offset + t == a.burn + 1) {
        need_rows(t + NS);
        trajectory(zs[0], lus[0], std::true_type{}, first, first);
        moved(1);
        rotate();
        handover(std::integral_constant<int, 1>{});
      }
      while (t + NU - 1 < t_end) {
        need_rows(t + NU - 1 + NS);
        quad_static_for<0, NU>([&](auto I) { trajectory(zs[I % NS], lus[I % NS], plain, I, first); });
        moved(NU);
        handover(std::integral_constant<int, NU>{});
      }
      while (t + NS - 1 < t_end) {
        need_rows(t + NS - 1 + NS);
        quad_static_for<0, NS>([&](auto I) { trajectory(zs[I], lus[I], plain, I, first); });
        moved(NS);
        handover(std::integral_constant<int, NS>{});
      }
      while (t < t_end) { need_rows(t + NS); trajectory(zs[0], lus[0], plain, first, first); moved(1); rotate(); handover(std::integral_constant<int, 1>{}); }
    } else {
      if (phase == 1 && t < t_end && a.traj_offset + t == a.burn + 1) {              // the Q2 trajectory opens the stored phase
        trajectory(zs[0], lus[0], std::true_type{}, first, first);
        rotate();
      }
      while (t + 2 * NS - 1 < t_end) {            // unrolled over the slots (twice): no register rotation on the hot path
#pragma unroll
        for (int i = 0; i < 2 * NS; ++i) trajectory(zs[i % NS], lus[i % NS], plain, first, first);
      }
      if (t + NS - 1 < t_end) {
#pragma unroll
        for (int i = 0; i < NS; ++i) trajectory(zs[i], lus[i], plain, first, first);
      }
      while (t < t_end) { trajectory(zs[0], lus[0], plain, first, first); rotate(); }
    }
  }
  if constexpr (ROWS) {                           // one more group: whether this wave's hand-over from the producers failed
    asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" :: "v"(lds), "v"(starved ? 1u : 0u) : "memory");
    return;
  }
  if constexpr (FUSED) {
    if (__builtin_expect(starved, 0)) {           // see QuadFused: the rows of this launch and the chain state become NaN
      qc = __builtin_nanf("");
      if (a.samples) {
        const size_t r0 = (size_t)max(a.traj_offset + n_burn - a.burn, 1);
        for (int tt = n_burn; tt < a.n_traj; ++tt) put((gwbytes_t)(a.samples + (r0 + (size_t)(tt - n_burn)) * C * D), qc);
      }
    }
  }
  put((gwbytes_t)a.theta, qc);
  if (a.reject_count && k == 0) a.reject_count[c] += a.n_traj - accepted;
}

// The row wave of an integrating wave (ROWS above): same lane, same chain, same coordinate.  It walks the groups of trajectories in
// the integrator's order, one barrier in front of each, and owns the output side.  In the burn-in phase it stores no row (the
// one-launch form rewrites the chain's slot of `theta` every trajectory; nobody reads those within the launch): only the final state.
// WT (tuning key "quad_rows_wt", the local and wide launches): the sample row element is stored WRITE-THROUGH at agent scope (a relaxed
// atomic store: global_store_dword ... sc1, a store the compiler tracks), so a launch's 12 MB of rows leave the XCD's L2 while the
// launch runs, not in the write-back of dirty lines behind its last wave (profiles/r15a_quad_lead.txt).  Same value, same address;
// the final state, the reject count and a starved launch's NaN rows stay plain stores.  -DQUAD_ABLATE_ROWSTORE (developer builds,
// timing only, wrong samples): the row wave stores no sample row - the ceiling of WT.
template <int D, int LB, bool LOCAL = false, bool WIDE = false>
__device__ __forceinline__ void quad_rows_body(const GaussArgs<float>& a, const float* __restrict__ eig, const int64_t gt, uint32_t lds,
                                               const bool wt = false) {
  typedef float T;
  constexpr int NS = quad_fused_ns(LB, true), NU = quad_nu(LB, NS, true);
  const bool on = (gt >> 2) < a.C;
  const int64_t c = on ? gt >> 2 : a.C - 1;
  const int k = (int)(gt & 3);
  const int kk = k < D ? k : 0;                 // a dummy lane mirrors lane 0 (same address, same value)
  const T mu = a.mu[kk];
  T Qrow[D];
#pragma unroll
  for (int j = 0; j < D; ++j) Qrow[j] = eig[EIG_TOUT(D) + kk * D + j];
  auto to_q = [&](T y) {                         // quad_body's: the same instructions in the same order
    T q = mu;
    asm volatile("s_nop 1" : "+v"(y));
#pragma unroll
    for (int j = 0; j < D; ++j)
      asm volatile("v_fmac_f32_dpp %0, %1, %2 quad_perm:[%3,%3,%3,%3] row_mask:0xf bank_mask:0xf"
                   : "+v"(q) : "v"(y), "v"(Qrow[j]), "n"(j));
    return q;
  };
  const size_t C = (size_t)a.C;
  const size_t el = (size_t)c * D + kk;
  T qc = a.theta[el];
  int32_t accepted = 0;
  const uint32_t lds_both = 2u * lds + (uint32_t)(NU * 256);
  const int n_burn = a.samples ? min(max(a.burn - a.traj_offset + 1, 0), a.n_traj) : a.n_traj;
  T* row = nullptr;
  auto take = [&](T m, bool q2) {               // one trajectory's message
    const bool acc = __builtin_bit_cast(uint32_t, m) != QUAD_ROWS_REJECT;
    const T q = to_q(m);                         // (every lane: the DPP operands come from the quad's other lanes)
    qc = acc ? q : qc;
    accepted += acc ? 1 : 0;
    if (q2 && !acc) qc = a.theta_init[el];       // Q2: back to params_init itself
#if defined(QUAD_ABLATE_ROWSTORE)
    if (row) row += C * D;
#else
    if (row) {
      if (on) {
        if (wt) __hip_atomic_store(row + el, qc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else row[el] = qc;
      }
      row += C * D;
    }
#endif
  };
  auto group = [&](auto G, bool q2) {
    asm volatile("s_barrier" ::: "memory");      // the integrator has filled this buffer
    constexpr int g = decltype(G)::value;
    if constexpr (WIDE && g % 4 == 0) {           // one 16-byte read per block of four positions (quad_body: WIDE)
      for (int i = 0; i < g; i += 4) {
        typedef float V4f __attribute__((ext_vector_type(4)));
        V4f m;
        asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(m) : "v"(lds + (uint32_t)i * 256u) : "memory");
        take(m[0], false); take(m[1], false); take(m[2], false); take(m[3], false);
      }
    } else if constexpr (g % 4 == 0) {
      for (int i = 0; i < g; i += 4) {
        T m0, m1, m2, m3;
        asm volatile("ds_read_b32 %0, %4\n\tds_read_b32 %1, %4 offset:256\n\tds_read_b32 %2, %4 offset:512\n\tds_read_b32 %3, %4 offset:768\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(m0), "=&v"(m1), "=&v"(m2), "=&v"(m3) : "v"(lds + (uint32_t)i * 256u) : "memory");
        take(m0, false); take(m1, false); take(m2, false); take(m3, false);
      }
    } else {
      for (int i = 0; i < g; ++i) {
        T m;
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(m) : "v"(lds + (uint32_t)i * 256u) : "memory");
        take(m, q2);
      }
    }
    lds = lds_both - lds;
  };
  std::integral_constant<int, 1> one;
  int t = 0;
  if constexpr (LOCAL) {                          // the local launch's sequence (its first barrier publishes records: not this wave's business)
    asm volatile("s_barrier" ::: "memory");
    quad_local_groups<NS, NU>(a, [&](int t0, int phase, auto G, auto q2) {
      if (phase == 1 && !row) row = a.samples + (size_t)max(a.traj_offset + t0 - a.burn, 1) * C * D;      // (the stored phase is empty without a.samples)
      group(G, decltype(q2)::value);
    });
  } else
  for (int phase = 0; phase < 2; ++phase) {
    const int t_end = phase == 0 ? n_burn : a.n_traj;
    if (phase == 1) {
      row = a.samples ? a.samples + (size_t)max(a.traj_offset + t - a.burn, 1) * C * D : nullptr;
      if (t < t_end && a.traj_offset + t == a.burn + 1) { group(one, true); t += 1; }
    }
    while (t + NU - 1 < t_end) { group(std::integral_constant<int, NU>{}, false); t += NU; }
    while (t + NS - 1 < t_end) { group(std::integral_constant<int, NS>{}, false); t += NS; }
    while (t < t_end) { group(one, false); t += 1; }
  }
  uint32_t starved;
  asm volatile("s_barrier\n\tds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(starved) : "v"(lds) : "memory");
  if (QUAD_ABLATE_WIDE_ON && LOCAL) starved = 0u;      // (the ceiling build's rings hold junk)
  if (__builtin_expect(starved != 0u, 0)) {     // see QuadFused: the rows of this launch and the chain state become NaN
    qc = __builtin_nanf("");
    if (a.samples && on) {
      const size_t r0 = (size_t)max(a.traj_offset + n_burn - a.burn, 1);
      for (int tt = n_burn; tt < a.n_traj; ++tt) a.samples[(r0 + (size_t)(tt - n_burn)) * C * D + el] = qc;
    }
  }
  if (on) {
    a.theta[el] = qc;
    if (a.reject_count && k == 0) a.reject_count[c] += a.n_traj - accepted;
  }
}

template <int D, bool DIAG, int LB, int VAR = 0>
__global__ __launch_bounds__(64) void hmc_gauss_quad_kernel(GaussArgs<float> a, const float* __restrict__ eig) {
  quad_body<D, DIAG, LB, VAR, false>(a, eig, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, QuadFused{nullptr, 1, 0u, 0, nullptr, 0});
}

// one record (csrc: rng_fill_small_kernel's body): the draws of trajectory n of global chain `chain`, rotated into the eigenbasis, and
// 2 log u in element D.  The ONE body of the record's arithmetic: the cross-block producers and the local launch's producer waves
// both call it, so their records are the same bits.
template <int D>
__device__ __forceinline__ void quad_make_record(uint64_t seed, uint64_t chain, uint32_t n, const float* __restrict__ eig,
                                                 float (&rec)[rec_elems<float, D>()]) {
  typedef float T;
  constexpr int W = rec_elems<T, D>();
  T z[D], lu;
  draw_inline<T, D>(seed, chain, n, z, lu);
#pragma unroll
  for (int i = 0; i < W; ++i) rec[i] = 0;
#pragma unroll
  for (int kk = 0; kk < D; ++kk) {
    T acc = eig[EIG_QT(D) + kk * D + 0] * z[0];
#pragma unroll
    for (int i = 1; i < D; ++i) acc = fma(eig[EIG_QT(D) + kk * D + i], z[i], acc);
    rec[kk] = acc;
  }
  rec[D] = 2.0f * lu;
}
template <int D>
__device__ __forceinline__ void quad_fill_record(float* __restrict__ ws, int64_t idx, int64_t C, int traj_offset, uint64_t seed,
                                                 uint64_t chain_offset, const float* __restrict__ eig) {
  typedef float T;
  constexpr int W = rec_elems<T, D>();
  const int64_t t = idx / C, c = idx - t * C;
  T rec[W];
  quad_make_record<D>(seed, chain_offset + (uint64_t)c, (uint32_t)(traj_offset + (int)t), eig, rec);
  // write-through stores at agent scope (sc1): the record is in memory, visible to the consumers' XCDs, once the store is
  // acknowledged - no L2 write-back per producer block (a buffer_wbl2 per 64 records made the producers 40x slower)
  // (one 16-byte store with the agent-scope bit: four dword stores quadrupled the write transactions)
  typedef float V4f __attribute__((ext_vector_type(4)));
  static_assert(W % 4 == 0, "records are whole 16-byte words");
#pragma unroll
  for (int i = 0; i < W / 4; ++i) {
    const V4f v = {rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3]};
    const __attribute__((address_space(1))) V4f* dst = (const __attribute__((address_space(1))) V4f*)(ws + idx * W + 4 * i);
    // (s_nop: a store wider than 8 bytes reads its data registers after issue; the compiler pads that hazard for stores it
    //  knows, not for inline assembly - without it the next VALU write into v's registers corrupted the record: D = 4 caught it)
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 2" :: "v"(dst), "v"(v) : "memory");
  }
}

// consumers (blocks [0, nc): the quad kernel's body) and producers (the blocks behind them, chunk-major: block b writes the
// 64-record slice b % spc of chunk b / spc) in ONE launch.  `done` counts the consumer blocks that finished: the last one
// zeroes the counters for the next launch (no memset node, nothing the host has to track: the launch stays graph-capturable).
constexpr int QUAD_FUSED_NT = 256;         // four waves per block: a producer block counts itself ONCE per chunk (the counter of a chunk
                                           // is one address: its atomic adds serialise - 512 one-wave producers were 3x slower than 128)
// NI (tuning key "quad_rows"): 0 = every consumer wave integrates and stores its rows itself (QUAD_FUSED_NT threads); NI > 0 = a block
// of 2 NI waves, waves [0, NI) integrate, wave NI + w is the row wave of wave w (quad_body: ROWS).  A producer block writes the same
// 256-record slices whatever the block size, so the records, the chunk counters and their target do not depend on NI.
#ifndef QUAD_ROWS_NI
#define QUAD_ROWS_NI 2                     // with two pairs per block the integrating waves and the row waves sit on different SIMDs of the
#endif                                     // CU (waves of a workgroup are dealt out round robin) and the block size is the producers' own
constexpr int quad_fused_threads(int NI) { return NI > 0 ? 128 * NI : QUAD_FUSED_NT; }
template <int D, int LB, int NI = 0>
__global__ __launch_bounds__(quad_fused_threads(NI)) void hmc_gauss_quad_fused_kernel(GaussArgs<float> a, const float* __restrict__ eig, QuadFused fz,
                                                                                      int nc, int spc, uint32_t* done) {
  constexpr int NT = quad_fused_threads(NI);
  if ((int)blockIdx.x >= nc) {
    // producer block b of spc: its slices of every chunk, chunk by chunk; one count per block and chunk
    const int b = (int)blockIdx.x - nc;
    if (fz.starve) return;                                                        // debug key "quad_starve": a producer that is never scheduled
    const int64_t per_chunk = (int64_t)fz.ch * a.C, total = (int64_t)a.n_traj * a.C;
    for (int chn = 0; chn < fz.nchunks; ++chn) {
      const int64_t base = (int64_t)chn * per_chunk, end = min(base + per_chunk, total);
      for (int sub = threadIdx.x; sub < QUAD_FUSED_NT; sub += NT)               // (NT = QUAD_FUSED_NT: once)
        for (int64_t idx = base + (int64_t)b * QUAD_FUSED_NT + sub; idx < end; idx += (int64_t)spc * QUAD_FUSED_NT)
          quad_fill_record<D>(a.ws_z, idx, a.C, a.traj_offset, a.seed, a.chain_offset, eig);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                          // this wave's records are acknowledged ...
      __syncthreads();                                                          // ... and so are the block's other waves' ...
      if (threadIdx.x == 0) __hip_atomic_fetch_add(fz.flags + chn, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ... before they are counted
    }
    return;
  }
  if constexpr (NI > 0) {
    constexpr int NS = quad_fused_ns(LB, true), NU = quad_nu(LB, NS, true);
    __shared__ float ring[NI * 2 * NU * 64];       // per integrating wave: two buffers of NU positions x 64 lanes
    const int wave = (int)(threadIdx.x >> 6), pair = wave < NI ? wave : wave - NI;
    const uint32_t lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)ring + (uint32_t)(pair * 2 * NU * 256) + (uint32_t)(threadIdx.x & 63) * 4u;
    const int64_t gt = ((int64_t)blockIdx.x * NI + pair) * 64 + (threadIdx.x & 63);
    if (wave >= NI) { quad_rows_body<D, LB>(a, eig, gt, lds); return; }
    __builtin_amdgcn_s_setprio(3);
    quad_body<D, false, LB, 7, true, true>(a, eig, gt, fz, lds);
  } else {
    __builtin_amdgcn_s_setprio(3);                 // a consumer's time is its issue rate: it goes first where a producer shares its SIMD
#if defined(QUAD_ABLATE_ROWS)      // timing only (profiles/r07a_quad_rows.txt): the integrator's side of ROWS with nobody reading the ring - the ceiling of the row wave
    constexpr int NS = quad_fused_ns(LB, true), NU = quad_nu(LB, NS, true);
    __shared__ float ring[4 * 2 * NU * 64];
    quad_body<D, false, LB, 7, true, true>(a, eig, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, fz,
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)ring + (uint32_t)((threadIdx.x >> 6) * 2 * NU * 256) + (uint32_t)(threadIdx.x & 63) * 4u);
#else
    quad_body<D, false, LB, 7, true>(a, eig, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, fz);
#endif
  }
  if (threadIdx.x == 0) {
    const uint32_t old = __hip_atomic_fetch_add(done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (old == (uint32_t)nc - 1u) {                                             // every consumer has read every chunk
      for (int i = 0; i < fz.nchunks; ++i) __hip_atomic_store(fz.flags + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(done, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}


// LOCAL (tuning key "quad_local", default 1; D <= 3): the records of a block's chains are drawn by producer waves of THAT block and
// handed over through LDS - no record travels through memory, no chunk counter, no poll, no wait for chunk 0, and the launch does
// not depend on any other block being resident (the HAND-OVER FAILURE of QuadFused cannot happen: waves of one workgroup are
// co-resident by construction).  One block = 16 chains, four waves, one per SIMD:
//   wave 0     integrates (quad_body: ROWS, LOCAL): its record element is a ds_read_b32 at lane base + position x 256
//   wave 1     its row wave (quad_rows_body)
//   waves 2-3  produce: lane (position % 8, chain) computes quad_make_record's record - the cross-block producer's arithmetic - and
//              writes it with one 16-byte LDS write to [position][chain]
//   ring       next to the message ring, two record buffers of one pass (NU positions x 16 chains x 16 bytes)
//   hand-over  the barrier per group of the row-wave protocol, joined by the producers: while the integrator runs group g they fill
//              buffer (g + 1) % 2 with the records of group g + 1, and the barrier between the two groups publishes it; one more
//              barrier in front of the first group.  All roles walk quad_local_groups.
// Results are bit-identical to the cross-block launch (tests/test_gpu_quad_local.py).  -DQUAD_ABLATE_LOCAL (developer builds, timing
// only, wrong samples: profiles/r08a_quad_local.txt): the producer waves draw nothing - the ceiling of the integrator's side.
// WIDE (quad_body: WIDE): element k of the record of position p goes to the integrating lane chain * 4 + k of block p >> 2, slot p & 3 -
// four dwords 16 bytes apart; a sweep of eight positions is two blocks.
// The sweep: lane `pl` of `nl` producer lanes draws positions pl / 16, + nl / 16, ... of a group for chain pl % 16 (128 lanes: eight
// positions of 16 chains per sweep); pl < 0: this wave draws nothing and only walks the groups.
// LEAD (hmc_gauss_quad_lead_kernel, tuning key "quad_lead"): the groups up to and including the launch's first full pass of NU are
// drawn with the sweep (pl_lead, nl_lead) - more lanes: the integrating wave waits for exactly these records with nothing to do -
// and the groups behind it with (pl, nl); both sweeps put a record where the integrating wave reads it.  pl_lead % 16 == pl % 16.
// INVARIANT: which lanes draw is the only thing a sweep decides.  Every wave that runs this function - drawing or not, chains past
// a.C or not, a launch shorter than one group or not - executes one "s_waitcnt lgkmcnt(0) ; s_barrier" per group of
// quad_local_groups, in that order, and the two closing barriers: the barrier sequence of every role is a function of the launch
// arguments alone, whatever the sweeps are.
template <int D, int LB, bool WIDE = false>
__device__ __forceinline__ void quad_local_produce(const GaussArgs<float>& a, const float* __restrict__ eig, const int64_t c0, const uint32_t recl,
                                                   const int pl, const int nl, const int pl_lead, const int nl_lead) {
  constexpr int NS = quad_fused_ns(LB, true), NU = quad_nu(LB, NS, true);
  static_assert(rec_elems<float, D>() == 4, "one 16-byte record");
  typedef float V4f __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) V4f* lvec_t;
  typedef __attribute__((address_space(3))) float* lflt_t;
  (void)(lvec_t)nullptr;
  const int chain = pl_lead & 15;
  const int64_t c = min(c0 + chain, a.C - 1);                                   // (past a.C: the last chain again, as the integrator does)
  const uint64_t gchain = a.chain_offset + (uint64_t)c;
  uint32_t buf = recl;                                                          // the record buffer being filled
  const uint32_t buf_both = 2u * recl + (uint32_t)(NU * 256);
  bool lead = true;
  quad_local_groups<NS, NU>(a, [&](int t0, int, auto G, auto) {
#if !defined(QUAD_ABLATE_LOCAL)
    const int l = lead ? pl_lead : pl, step = (lead ? nl_lead : nl) >> 4;       // (step: a multiple of four positions - whole blocks of WIDE)
    const int p0 = l >= 0 ? l >> 4 : NU;                                        // (NU: past every group)
    const uint32_t dst = buf + (WIDE ? (uint32_t)((p0 >> 2) * 1024 + chain * 64 + (p0 & 3) * 4) : (uint32_t)(p0 * 256 + chain * 16));
    for (int p = p0; p < decltype(G)::value; p += step) {                       // (p < NU: inside the buffer)
      float rec[4];
      quad_make_record<D>(a.seed, gchain, (uint32_t)(a.traj_offset + t0 + p), eig, rec);
      if constexpr (WIDE) {
        const lflt_t w = (lflt_t)(uintptr_t)(dst + (uint32_t)((p - p0) * 256));      // (four positions on: one block of 1024 bytes)
        w[0] = rec[0]; w[4] = rec[1]; w[8] = rec[2]; w[12] = rec[3];
      } else {
        *(lvec_t)(uintptr_t)(dst + (uint32_t)((p - p0) * 256)) = V4f{rec[0], rec[1], rec[2], rec[3]};
      }
    }
#endif
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");          // publishes this group's records
    buf = buf_both - buf;
    if (decltype(G)::value == NU) lead = false;
  });
  asm volatile("s_barrier\n\ts_barrier" ::: "memory");                          // the last group's hand-over and the status message: the other roles'
}
template <int D, int LB>
__global__ __launch_bounds__(256) void hmc_gauss_quad_local_kernel(GaussArgs<float> a, const float* __restrict__ eig, int wt) {
  constexpr int NS = quad_fused_ns(LB, true), NU = quad_nu(LB, NS, true);
  __shared__ __attribute__((aligned(16))) float ring[2 * NU * 64 + 2 * NU * 64];      // messages (64 lanes x 4 bytes) | records (16 chains x 16 bytes), two passes each
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const uint32_t msgs = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)ring, recs = msgs + (uint32_t)(2 * NU * 256);
  const int64_t gt = (int64_t)blockIdx.x * 64 + lane;
  if (wave == 0) {
    __builtin_amdgcn_s_setprio(3);
    quad_body<D, false, LB, 7, true, true, true>(a, eig, gt, QuadFused{nullptr, 1, 0u, 0, nullptr, 0}, msgs + (uint32_t)lane * (QUAD_ABLATE_WIDE_ON ? 16u : 4u), recs + (uint32_t)lane * (QUAD_ABLATE_WIDE_ON ? 16u : 4u));
  }
  else if (wave == 1) quad_rows_body<D, LB, true>(a, eig, gt, msgs + (uint32_t)lane * 4u, wt != 0);
  else quad_local_produce<D, LB>(a, eig, (int64_t)blockIdx.x * 16, recs, (int)threadIdx.x - 128, 128, (int)threadIdx.x - 128, 128);
}
// WIDE (tuning key "quad_wide"): the local launch - the same roles, rings of the same sizes, the same groups and barriers - with
// 16-byte hand-overs per block of four positions (quad_body: WIDE); a lane's base in a block of either ring is lane x 16 bytes.
// Results are bit-identical to the local launch (tests/test_gpu_quad_wide.py).
// LEAD (tuning key "quad_lead", hmc_gauss_quad_lead_kernel): the wide launch with 512 threads.  The launch's lead-in is the time the
// producers need for the first full pass - 32 positions x 16 chains, four sweeps of waves 2-3 - while the integrating wave, done
// with the lead group after one eighth of that, and the row wave stand at a barrier.  Waves 4-7 draw their share of the groups
// up to and including that pass (quad_local_produce: LEAD): 384 lanes, 24 positions per sweep, waves 4-5 (the SIMDs of the two
// idle roles) first in the sweep, so the pass is two wave-sweeps on each SIMD instead of four on two.  Behind it they draw
// nothing and walk the groups to the end with everybody's barriers; they never leave early.  Same records in the same places:
// results are bit-identical to the 256-thread launch (tests/test_gpu_quad_lead.py).
template <int D, int LB, bool LEAD>
__device__ __forceinline__ void quad_wide_block(const GaussArgs<float>& a, const float* __restrict__ eig, const bool wt) {
  constexpr int NS = quad_fused_ns(LB, true), NU = quad_nu(LB, NS, true);
  static_assert(NS == 4 && NU % 4 == 0, "groups are whole blocks of four positions, or single ones");
  __shared__ __attribute__((aligned(16))) float ring[2 * NU * 64 + 2 * NU * 64];      // as the local launch's: messages | records, two passes each
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const uint32_t msgs = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)ring, recs = msgs + (uint32_t)(2 * NU * 256);
  const int64_t gt = (int64_t)blockIdx.x * 64 + lane;
  if (wave == 0) {
    __builtin_amdgcn_s_setprio(3);
    quad_body<D, false, LB, 7, true, true, true, true>(a, eig, gt, QuadFused{nullptr, 1, 0u, 0, nullptr, 0}, msgs + (uint32_t)lane * 16u, recs + (uint32_t)lane * 16u);
  }
  else if (wave == 1) quad_rows_body<D, LB, true, true>(a, eig, gt, msgs + (uint32_t)lane * 16u, wt);
  else if constexpr (LEAD) {
    const int lw = wave < 4 ? wave : (wave < 6 ? wave - 4 : wave - 2);               // place in the lead sweep: waves 4 5 2 3 6 7
    quad_local_produce<D, LB, true>(a, eig, (int64_t)blockIdx.x * 16, recs, wave < 4 ? (int)threadIdx.x - 128 : -1, 128, lw * 64 + lane, 384);
  }
  else quad_local_produce<D, LB, true>(a, eig, (int64_t)blockIdx.x * 16, recs, (int)threadIdx.x - 128, 128, (int)threadIdx.x - 128, 128);
}
template <int D, int LB>
__global__ __launch_bounds__(256) void hmc_gauss_quad_wide_kernel(GaussArgs<float> a, const float* __restrict__ eig, int wt) {
  quad_wide_block<D, LB, false>(a, eig, wt != 0);
}
template <int D, int LB>
__global__ __launch_bounds__(512) void hmc_gauss_quad_lead_kernel(GaussArgs<float> a, const float* __restrict__ eig, int wt) {
  quad_wide_block<D, LB, true>(a, eig, wt != 0);
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

// =============================================================================================
// dispatch
// =============================================================================================
// the quad kernel's eligibility
constexpr int QUAD_FUSED_CHUNKS = 64, QUAD_FUSED_OFF = 56;      // (capacity; "quad_chunks" of them are used)
int g_quad_chunks = 8;       // tuning key "quad_chunks": chunks per fused launch (<= 64; measured 4 ... 60: profiles/r04k_quad_fused_sweep.txt)      // counters in the free tail of the eig block (D <= 4 uses 52 of 128 elements)
int g_quad_producers = 64;   // tuning key "quad_producers": producer blocks (four waves each) of the fused launch per 1024 chains
int g_quad_starve = 0;       // debug key "quad_starve": 1 = the producers of the fused launch leave without producing (exercises the consumers' bounded wait)
constexpr int QUAD_STATUS_OFF = QUAD_FUSED_OFF + QUAD_FUSED_CHUNKS + 1;         // element of the eig block that holds the sticky status word
static_assert(QUAD_STATUS_OFF < 128, "the status word lives in the eig block's free tail");
int g_quad_rows = 1;         // tuning key "quad_rows" (default 1): the fused launch hands the sample rows to row waves through LDS (quad_body: ROWS); 0 = every consumer wave stores its own
int g_quad_local = 1;        // tuning key "quad_local" (default 1): with "quad_rows" and D <= 3 the records are drawn by producer waves of the consumer's own block (hmc_gauss_quad_local_kernel); 0 = producer blocks behind the consumers', the parity partner
int g_quad_wide = 1;         // tuning key "quad_wide" (default 1): the local launch hands records and messages over in 16-byte LDS accesses per block of four trajectories (hmc_gauss_quad_wide_kernel); 0 = the 4-byte hand-overs of hmc_gauss_quad_local_kernel, the parity partner
int g_quad_rows_wt = 1;      // tuning key "quad_rows_wt" (default 1): the row wave of the local and wide launches stores the sample rows write-through at agent scope (quad_rows_body: WT); 0 = plain stores, the parity partner
int g_quad_lead = 1;         // tuning key "quad_lead" (default 1): the wide launch runs with 512 threads, waves 4-7 drawing records up to the first full pass (hmc_gauss_quad_lead_kernel); 0 = the 256-thread launch, the parity partner
int g_quad_wide_launches = 0; // debug key "quad_wide_launches": launches of hmc_gauss_quad_wide_kernel since the keys were last reset (the route string does not tell the two local launches apart; tests/test_gpu_quad_wide.py reads it)
int g_quad_fused = 1;        // tuning key "quad_fused" (default 1): records produced inside the trajectory launch (prepared workspaces only); 0 = a pre-draw launch in front of it
template <typename T> static bool eig_block_prepared(const GaussArgs<T>& a, int mass_kind);
template <typename T> static bool quad_route(const GaussArgs<T>& a);
// the fused launch: the quad route with the default instance on a PREPARED workspace (its counters were zeroed by the preparation
// and are zeroed again by every fused launch's last consumer), rows that are whole 128-byte lines, at least one trajectory per chunk
template <typename T> static bool quad_fused_route(const GaussArgs<T>& a, int mass_kind, bool diag) {
  if constexpr (sizeof(T) != 4) return false;
  else {
    // (up to 4096 chains: the regime where the trajectory kernel leaves most of the chip to the producers)
    if (!g_quad_fused || diag || g_quad_variant != 7 || !quad_route(a) || a.D > 4 || a.C > 4096 || a.n_traj < 8) return false;
    const int W = ((a.D + 1 + 3) / 4) * 4;
    if (((int64_t)a.C * W * 4) % 128 != 0 || ((uintptr_t)a.ws_z % 128) != 0) return false;
    return eig_block_prepared(a, mass_kind);
  }
}
template <typename T> static bool quad_route(const GaussArgs<T>& a) {
  return sizeof(T) == 4 && a.D <= 4 && a.ws_z && a.ws_logu && g_gauss_eig >= 1 && g_gauss_eig != 2 &&
         a.C <= g_quad_max_chains && a.C <= (1 << 24);
}
template <typename T, int D, int MASS> void launch_small(const GaussArgs<T>& a, bool lf_only, hipStream_t s) {
  int block = g_small_chains_per_block > 0 ? g_small_chains_per_block : 64;
  const int grid = (int)((a.C + block - 1) / block);
  if (lf_only) { leapfrog_gauss_small_kernel<T, D, MASS><<<grid, block, 0, s>>>(a); return; }
  const bool diag = a.H_old || a.H_new || a.accept;
  if (a.ws_z && a.ws_logu) {      // eigenbasis route, any mass kind (whitened; a.ws_logu = the eig block)
    if constexpr (sizeof(T) == 4 && D <= 4) {
      if (quad_route(a)) {   // latency regime: a quad per chain (32-bit lane offsets)
        const int qgrid = (int)((a.C * 4 + 63) / 64);
        profile_begin(s);
        const int lb = g_gauss_eig == 3 ? 0 : a.L;       // gauss_eig = 3: the any-L instance (tests compare the two)
        note_route("hmc_gauss_quad_kernel<%d,%s,%d>", D, diag ? "true" : "false", diag ? 0 : (lb == 25 || lb == 10 || lb == 5) ? lb : 0);
        if (quad_fused_route(a, MASS, diag)) {
          // one launch: consumers + producers (see quad_body / hmc_gauss_quad_fused_kernel)
          constexpr int W = rec_elems<T, D>();
          const int lbv = (lb == 25 || lb == 10 || lb == 5) ? lb : 0;
          QuadFused fz;
          const int nch = g_quad_chunks < 1 ? 1 : (g_quad_chunks > QUAD_FUSED_CHUNKS ? QUAD_FUSED_CHUNKS : g_quad_chunks);
          fz.ch = (a.n_traj + nch - 1) / nch;
          fz.nchunks = (a.n_traj + fz.ch - 1) / fz.ch;
          int spc = (int)(((int64_t)fz.ch * a.C + QUAD_FUSED_NT - 1) / QUAD_FUSED_NT);   // producer blocks (four waves each): at most
          const int pmax = g_quad_producers * (int)((a.C + 1023) / 1024);                 // g_quad_producers per 1024 chains, each walks
          if (spc > pmax) spc = pmax;                                                     // its slices of every chunk
          fz.target = (uint32_t)spc;
          constexpr int NI = QUAD_ROWS_NI;
          const int cpb = g_quad_rows ? 64 * NI : QUAD_FUSED_NT;                           // chain lanes per consumer block ("quad_rows": NI integrating waves + NI row waves)
          const int qgrid = (int)((a.C * 4 + cpb - 1) / cpb);                              // consumer blocks of this launch shape
          fz.flags = reinterpret_cast<uint32_t*>(a.ws_logu + QUAD_FUSED_OFF);
          uint32_t* done = fz.flags + QUAD_FUSED_CHUNKS;
          fz.err = done + 1;                                                                  // the sticky status word (QUAD_STATUS_OFF)
          fz.starve = g_quad_starve;
          (void)W;
          note_route("hmc_gauss_quad_fused_kernel<%d,%d>", D, lbv);
          const int fgrid = qgrid + spc;
          // "quad_starve" emulates a producer BLOCK that is never scheduled - a failure the local launch cannot have - so it selects the cross-block launch
          if (D <= 3 && g_quad_rows && g_quad_local && !g_quad_starve) {
            if constexpr (D <= 3) {
              const int lgrid = (int)((a.C + 15) / 16);                                       // 16 chains per block; the record area of the workspace stays unused
              const int wt = g_quad_rows_wt ? 1 : 0;                                          // write-through sample rows (quad_rows_body: WT)
              if (g_quad_wide && g_quad_lead) {                                               // ... with waves 4-7 drawing in the lead-in (quad_wide_block: LEAD)
                ++g_quad_wide_launches;
                if (lbv == 25) hmc_gauss_quad_lead_kernel<D, 25><<<lgrid, 512, 0, s>>>(a, a.ws_logu, wt);
                else if (lbv == 10) hmc_gauss_quad_lead_kernel<D, 10><<<lgrid, 512, 0, s>>>(a, a.ws_logu, wt);
                else if (lbv == 5) hmc_gauss_quad_lead_kernel<D, 5><<<lgrid, 512, 0, s>>>(a, a.ws_logu, wt);
                else hmc_gauss_quad_lead_kernel<D, 0><<<lgrid, 512, 0, s>>>(a, a.ws_logu, wt);
              }
              else if (g_quad_wide) {                                                         // 16-byte hand-overs (quad_body: WIDE)
                ++g_quad_wide_launches;
                if (lbv == 25) hmc_gauss_quad_wide_kernel<D, 25><<<lgrid, 256, 0, s>>>(a, a.ws_logu, wt);
                else if (lbv == 10) hmc_gauss_quad_wide_kernel<D, 10><<<lgrid, 256, 0, s>>>(a, a.ws_logu, wt);
                else if (lbv == 5) hmc_gauss_quad_wide_kernel<D, 5><<<lgrid, 256, 0, s>>>(a, a.ws_logu, wt);
                else hmc_gauss_quad_wide_kernel<D, 0><<<lgrid, 256, 0, s>>>(a, a.ws_logu, wt);
              }
              else if (lbv == 25) hmc_gauss_quad_local_kernel<D, 25><<<lgrid, 256, 0, s>>>(a, a.ws_logu, wt);
              else if (lbv == 10) hmc_gauss_quad_local_kernel<D, 10><<<lgrid, 256, 0, s>>>(a, a.ws_logu, wt);
              else if (lbv == 5) hmc_gauss_quad_local_kernel<D, 5><<<lgrid, 256, 0, s>>>(a, a.ws_logu, wt);
              else hmc_gauss_quad_local_kernel<D, 0><<<lgrid, 256, 0, s>>>(a, a.ws_logu, wt);
            }
          }
          else if (g_quad_rows) {
            constexpr int NT = quad_fused_threads(NI);
            if (lbv == 25) hmc_gauss_quad_fused_kernel<D, 25, NI><<<fgrid, NT, 0, s>>>(a, a.ws_logu, fz, qgrid, spc, done);
            else if (lbv == 10) hmc_gauss_quad_fused_kernel<D, 10, NI><<<fgrid, NT, 0, s>>>(a, a.ws_logu, fz, qgrid, spc, done);
            else if (lbv == 5) hmc_gauss_quad_fused_kernel<D, 5, NI><<<fgrid, NT, 0, s>>>(a, a.ws_logu, fz, qgrid, spc, done);
            else hmc_gauss_quad_fused_kernel<D, 0, NI><<<fgrid, NT, 0, s>>>(a, a.ws_logu, fz, qgrid, spc, done);
          }
          else if (lbv == 25) hmc_gauss_quad_fused_kernel<D, 25><<<fgrid, QUAD_FUSED_NT, 0, s>>>(a, a.ws_logu, fz, qgrid, spc, done);
          else if (lbv == 10) hmc_gauss_quad_fused_kernel<D, 10><<<fgrid, QUAD_FUSED_NT, 0, s>>>(a, a.ws_logu, fz, qgrid, spc, done);
          else if (lbv == 5) hmc_gauss_quad_fused_kernel<D, 5><<<fgrid, QUAD_FUSED_NT, 0, s>>>(a, a.ws_logu, fz, qgrid, spc, done);
          else hmc_gauss_quad_fused_kernel<D, 0><<<fgrid, QUAD_FUSED_NT, 0, s>>>(a, a.ws_logu, fz, qgrid, spc, done);
        }
        else if (!diag && (g_quad_variant == 3 || g_quad_variant == 7) && a.C <= (1 << 20)) {
          // "quad_variant": 3 = uniform bases + 32-bit lane offsets, no NaN guard; 7 = also the fused row / butterfly block
          const int lbv = (lb == 25 || lb == 10 || lb == 5) ? lb : 0;
          note_route("hmc_gauss_quad_kernel<%d,false,%d,%d>", D, lbv, g_quad_variant);
          if (g_quad_variant == 3) {
            if (lbv == 25) hmc_gauss_quad_kernel<D, false, 25, 3><<<qgrid, 64, 0, s>>>(a, a.ws_logu);
            else if (lbv == 10) hmc_gauss_quad_kernel<D, false, 10, 3><<<qgrid, 64, 0, s>>>(a, a.ws_logu);
            else if (lbv == 5) hmc_gauss_quad_kernel<D, false, 5, 3><<<qgrid, 64, 0, s>>>(a, a.ws_logu);
            else hmc_gauss_quad_kernel<D, false, 0, 3><<<qgrid, 64, 0, s>>>(a, a.ws_logu);
          } else {
            if (lbv == 25) hmc_gauss_quad_kernel<D, false, 25, 7><<<qgrid, 64, 0, s>>>(a, a.ws_logu);
            else if (lbv == 10) hmc_gauss_quad_kernel<D, false, 10, 7><<<qgrid, 64, 0, s>>>(a, a.ws_logu);
            else if (lbv == 5) hmc_gauss_quad_kernel<D, false, 5, 7><<<qgrid, 64, 0, s>>>(a, a.ws_logu);
            else hmc_gauss_quad_kernel<D, false, 0, 7><<<qgrid, 64, 0, s>>>(a, a.ws_logu);
          }
        }
        else if (diag) hmc_gauss_quad_kernel<D, true, 0><<<qgrid, 64, 0, s>>>(a, a.ws_logu);
        else if (lb == 25) hmc_gauss_quad_kernel<D, false, 25><<<qgrid, 64, 0, s>>>(a, a.ws_logu);
        else if (lb == 10) hmc_gauss_quad_kernel<D, false, 10><<<qgrid, 64, 0, s>>>(a, a.ws_logu);
        else if (lb == 5) hmc_gauss_quad_kernel<D, false, 5><<<qgrid, 64, 0, s>>>(a, a.ws_logu);
        else hmc_gauss_quad_kernel<D, false, 0><<<qgrid, 64, 0, s>>>(a, a.ws_logu);
        profile_end(s);
        return;
      }
    }
    profile_begin(s);
    note_route("hmc_gauss_eig_kernel<%s,%d,%s>", sizeof(T) == 4 ? "float" : "double", D, diag ? "true" : "false");
    if (diag) hmc_gauss_eig_kernel<T, D, true><<<grid, block, 0, s>>>(a, a.ws_logu);
    else hmc_gauss_eig_kernel<T, D, false><<<grid, block, 0, s>>>(a, a.ws_logu);
    profile_end(s);
    return;
  }
  profile_begin(s);
  note_route("hmc_gauss_small_kernel<%s,%d,%d,%s,%s>", sizeof(T) == 4 ? "float" : "double", D, MASS, a.ws_z ? "true" : "false", diag ? "true" : "false");
  if (a.ws_z) {
    if (diag) hmc_gauss_small_kernel<T, D, MASS, true, true><<<grid, block, 0, s>>>(a);
    else hmc_gauss_small_kernel<T, D, MASS, true, false><<<grid, block, 0, s>>>(a);
  } else {
    if (diag) hmc_gauss_small_kernel<T, D, MASS, false, true><<<grid, block, 0, s>>>(a);
    else hmc_gauss_small_kernel<T, D, MASS, false, false><<<grid, block, 0, s>>>(a);
  }
  profile_end(s);
}
template <typename T, int D> void launch_small_m(const GaussArgs<T>& a, int kind, bool lf, hipStream_t s) {
  if (kind == HTA_MASS_NONE) launch_small<T, D, HTA_MASS_NONE>(a, lf, s);
  else if (kind == HTA_MASS_DIAG) launch_small<T, D, HTA_MASS_DIAG>(a, lf, s);
  else launch_small<T, D, HTA_MASS_FULL>(a, lf, s);
}
template <typename T, int R, int MASS> void launch_wave(const GaussArgs<T>& a, bool lf_only, hipStream_t s) {
  const int grid = (int)((a.C + GEN_WAVES - 1) / GEN_WAVES);
  const size_t lds = (size_t)GEN_WAVES * 64 * R * sizeof(T);
  if (lf_only) { leapfrog_gauss_wave_kernel<T, R, MASS><<<grid, 64 * GEN_WAVES, lds, s>>>(a); return; }
  profile_begin(s);
  note_route("hmc_gauss_wave_kernel<%s,%d,%d>", sizeof(T) == 4 ? "float" : "double", R, MASS);
  hmc_gauss_wave_kernel<T, R, MASS><<<grid, 64 * GEN_WAVES, lds, s>>>(a);
  profile_end(s);
}
// eigenbasis route of the wave kernel: identity mass, an eig area in the workspace, D within the Jacobi kernel's reach
template <typename T> static bool wave_eig_route(const GaussArgs<T>& a, int kind, bool lf_only) {
  return !lf_only && kind == HTA_MASS_NONE && g_gauss_eig && a.ws_logu && a.D <= 128;     // (R <= 2; fp64 beyond 99: the diagonalisation works in the workspace's slab)
}
// the eig area V | Vt | lam of the wave kernels' eigenbasis route, rounded to 16 bytes (a metric slab may follow)
static int64_t wave_eig_area_bytes(int D, int elem) { return (((int64_t)2 * D * D + D + 64) * elem + 15) & ~(int64_t)15; }
template <typename T, int R> int launch_wave_eig(const GaussArgs<T>& a, hipStream_t s) {
  const int D = a.D;
  T* V = a.ws_logu; T* Vt = V + (int64_t)D * D; T* lam = Vt + (int64_t)D * D;
  MetricArgsT<T> m0;
  memset(&m0, 0, sizeof(m0));
  m0.B = 1; m0.D = D; m0.metric = HTA_METRIC_SOFTABS; m0.Hs = a.P; m0.hs_stride = 0; m0.alpha = 1.0;
  m0.V_out = V; m0.lamraw_out = lam;
  m0.workspace_bytes = metric_eval_workspace_bytes(1, D, (int)sizeof(T));             // behind the eig area (hta_hmc_gaussian_workspace_bytes)
  m0.workspace = m0.workspace_bytes ? (char*)V + wave_eig_area_bytes(D, (int)sizeof(T)) : nullptr;
  const int rc = metric_eval<T>(m0, s);
  if (rc) return rc;
  if constexpr (sizeof(T) == 4) eig_polish_kernel<T><<<D, 128, 0, s>>>(a.P, V, lam, D);      // (float64 rotations leave |v|^2 - 1 at 1e-15: nothing to mend)
  transpose_kernel<T><<<(D * D + 255) / 256, 256, 0, s>>>(V, Vt, D);
  const int grid = (int)((a.C + GEN_WAVES - 1) / GEN_WAVES);
  const size_t lds = (size_t)GEN_WAVES * 64 * R * sizeof(T);
  profile_begin(s);
  note_route("hmc_gauss_wave_eig_kernel<%s,%d>", sizeof(T) == 4 ? "float" : "double", R);
  hmc_gauss_wave_eig_kernel<T, R><<<grid, 64 * GEN_WAVES, lds, s>>>(a, V);
  profile_end(s);
  return HTA_OK;
}
template <typename T, int R> void launch_wave_m(const GaussArgs<T>& a, int kind, bool lf, hipStream_t s) {
  if (kind == HTA_MASS_NONE) launch_wave<T, R, HTA_MASS_NONE>(a, lf, s);
  else if (kind == HTA_MASS_DIAG) launch_wave<T, R, HTA_MASS_DIAG>(a, lf, s);
  else launch_wave<T, R, HTA_MASS_FULL>(a, lf, s);
}

// ---- hta_hmc_gaussian_prepare: the eig block of a workspace filled once per TARGET ---------------------------------------
// eig_small_kernel (one wave, ~5 us + a launch gap: 3 % of a 1000-trajectory call at BASELINE config 2) depends on P and the mass
// operand only.  A caller that keeps sampling one target prepares its workspace once; a sample call whose eig block, P pointer,
// mass operand, D and element type match the preparation skips the kernel.  Keyed by (device, eig block pointer).
struct EigPrepared { const void* base; const void* P; const void* mass_factor; int mass_kind, D, elem; };
static std::mutex g_eig_mu;
static std::map<std::pair<int, const void*>, EigPrepared> g_eig_prepared;
static int eig_device() { int d = 0; (void)hipGetDevice(&d); return d; }
template <typename T> static bool eig_block_prepared(const GaussArgs<T>& a, int mass_kind) {
  std::lock_guard<std::mutex> lock(g_eig_mu);
  if (g_eig_prepared.empty()) return false;
  auto it = g_eig_prepared.find({eig_device(), (const void*)a.ws_logu});
  if (it == g_eig_prepared.end()) return false;
  const EigPrepared& e = it->second;
  return e.P == (const void*)a.P && e.mass_kind == mass_kind && e.D == a.D && e.elem == (int)sizeof(T) &&
         (mass_kind == HTA_MASS_NONE || e.mass_factor == (const void*)a.mass_factor);
}

// pre-draw pass: all momenta / log-uniforms of the launch, one thread per (trajectory, chain)
template <typename T, int D> static void launch_rng_fill_d(const GaussArgs<T>& a, int mass_kind, hipStream_t s) {
  const int64_t total = a.C * a.n_traj;
  int64_t g = (total + 255) / 256;
  if (g > g_fill_blocks) g = g_fill_blocks;
  if (a.ws_logu && !eig_block_prepared(a, mass_kind)) eig_small_kernel<T, D><<<1, 64, 0, s>>>(a.P, mass_kind, a.mass_factor, a.ws_logu);
  if (quad_fused_route(a, mass_kind, a.H_old || a.H_new || a.accept)) return;      // the records are produced inside the trajectory launch
  rng_fill_small_kernel<T, D><<<(int)g, 256, 0, s>>>(a.ws_z, a.C, a.n_traj, a.traj_offset, a.seed, a.chain_offset,
                                                     a.ws_logu, quad_route(a) ? (T)2 : (T)1);
}
template <typename T> static void launch_rng_fill(const GaussArgs<T>& a, int mass_kind, hipStream_t s) {
  switch (a.D) {
    case 1: launch_rng_fill_d<T, 1>(a, mass_kind, s); break;
    case 2: launch_rng_fill_d<T, 2>(a, mass_kind, s); break;
    case 3: launch_rng_fill_d<T, 3>(a, mass_kind, s); break;
    case 4: launch_rng_fill_d<T, 4>(a, mass_kind, s); break;
    case 5: launch_rng_fill_d<T, 5>(a, mass_kind, s); break;
    default: launch_rng_fill_d<T, 6>(a, mass_kind, s); break;
  }
}

template <typename T> int gaussian_dispatch(const GaussArgs<T>& a_in, int kind, bool lf_only, hipStream_t s) {
  GaussArgs<T> a = a_in;
  const char* who = lf_only ? "hta_hmc_gaussian_leapfrog" : "hta_hmc_gaussian_sample";
  HTA_REQUIRE(a.theta && a.P && a.mu, "%s: NULL state/model pointer", who);
  HTA_REQUIRE(a.C > 0 && a.D > 0 && a.D <= 1024, "%s: need C > 0 and 1 <= D <= 1024 (C=%lld D=%d)", who,
              (long long)a.C, a.D);
  HTA_REQUIRE(a.L >= 0, "%s: negative step count", who);
  HTA_REQUIRE(kind >= HTA_MASS_NONE && kind <= HTA_MASS_FULL, "%s: unknown mass kind %d", who, kind);
  HTA_REQUIRE(kind == HTA_MASS_NONE || (a.inv_mass && (lf_only || a.mass_factor)), "%s: mass operand is NULL", who);
  if (!lf_only) HTA_REQUIRE(a.theta_init && a.n_traj >= 0, "%s: bad trajectory arguments", who);
  if (lf_only) HTA_REQUIRE(a.p_io, "%s: momentum is NULL", who);
  if (a.n_traj == 0 && !lf_only) return HTA_OK;
  const int D = a.D;
  // f64 models past D=4 overflow the SGPR file (P alone is 2*D*D SGPRs) and would spill to scratch
  const int small_max = sizeof(T) == 8 ? 4 : 6;  // 2*D*D + 3*D wave-uniform operands must fit the SGPR file
  const bool reg_resident = D <= small_max && !g_force_general;
  if (!g_gauss_eig) a.ws_logu = nullptr;       // direct kernels on request
  if (a.ws_z && reg_resident && !lf_only) launch_rng_fill<T>(a, kind, s);
  else { a.ws_z = nullptr; if (reg_resident || lf_only) a.ws_logu = nullptr; }
  if (reg_resident) {
    switch (D) {
      case 1: launch_small_m<T, 1>(a, kind, lf_only, s); break;
      case 2: launch_small_m<T, 2>(a, kind, lf_only, s); break;
      case 3: launch_small_m<T, 3>(a, kind, lf_only, s); break;
      case 4: launch_small_m<T, 4>(a, kind, lf_only, s); break;
      case 5: if constexpr (sizeof(T) == 4) launch_small_m<T, 5>(a, kind, lf_only, s); break;
      default: if constexpr (sizeof(T) == 4) launch_small_m<T, 6>(a, kind, lf_only, s); break;
    }
  } else {
    const int R = (D + 63) / 64;
    if (wave_eig_route(a, kind, lf_only)) {
      const int rc = R <= 1 ? launch_wave_eig<T, 1>(a, s) : launch_wave_eig<T, 2>(a, s);
      if (rc) return rc;
    }
    else if (R <= 1) launch_wave_m<T, 1>(a, kind, lf_only, s);
    else if (R <= 2) launch_wave_m<T, 2>(a, kind, lf_only, s);
    else if (R <= 4) launch_wave_m<T, 4>(a, kind, lf_only, s);
    else if (R <= 8) launch_wave_m<T, 8>(a, kind, lf_only, s);
    else launch_wave_m<T, 16>(a, kind, lf_only, s);
  }
  HTA_CHECK_LAUNCH(who);
  return HTA_OK;
}

template <typename T>
int gaussian_prepare(const T* P, int mass_kind, const T* mass_factor, int64_t C, int D, int n_traj, void* workspace,
                     int64_t workspace_bytes, int64_t need, hipStream_t s) {
  const char* who = "hta_hmc_gaussian_prepare";
  HTA_REQUIRE(P && C > 0 && D > 0 && n_traj > 0, "%s: bad arguments", who);
  HTA_REQUIRE(mass_kind >= HTA_MASS_NONE && mass_kind <= HTA_MASS_FULL && (mass_kind == HTA_MASS_NONE || mass_factor),
              "%s: bad mass operand", who);
  HTA_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %lld bytes required", who, (long long)need);
  std::lock_guard<std::mutex> lock(g_eig_mu);
  // one preparation per workspace: an earlier one (another trajectory count = another eig block position) goes
  for (auto it = g_eig_prepared.begin(); it != g_eig_prepared.end();)
    it = (it->first.first == eig_device() && it->second.base == workspace) ? g_eig_prepared.erase(it) : std::next(it);
  const int small_max = sizeof(T) == 8 ? 4 : 6;
  if (D > small_max || !g_gauss_eig || g_force_general) return HTA_OK;      // no eig block on those routes: nothing to hoist
  T* eig = (T*)((char*)workspace + need) - EIG_ELEMS;
  switch (D) {
    case 1: eig_small_kernel<T, 1><<<1, 64, 0, s>>>(P, mass_kind, mass_factor, eig); break;
    case 2: eig_small_kernel<T, 2><<<1, 64, 0, s>>>(P, mass_kind, mass_factor, eig); break;
    case 3: eig_small_kernel<T, 3><<<1, 64, 0, s>>>(P, mass_kind, mass_factor, eig); break;
    case 4: eig_small_kernel<T, 4><<<1, 64, 0, s>>>(P, mass_kind, mass_factor, eig); break;
    case 5: eig_small_kernel<T, 5><<<1, 64, 0, s>>>(P, mass_kind, mass_factor, eig); break;
    default: eig_small_kernel<T, 6><<<1, 64, 0, s>>>(P, mass_kind, mass_factor, eig); break;
  }
  if (D <= 4 && sizeof(T) == 4) {       // the fused quad launch's chunk counters + consumer count live in the block's free tail
    if (hipMemsetAsync(eig + QUAD_FUSED_OFF, 0, (QUAD_FUSED_CHUNKS + 2) * sizeof(uint32_t), s) != hipSuccess) {
      set_error("%s: hipMemsetAsync failed", who);
      return HTA_ERR_LAUNCH;
    }
  }
  HTA_CHECK_LAUNCH(who);
  g_eig_prepared[{eig_device(), (const void*)eig}] = EigPrepared{workspace, P, mass_factor, mass_kind, D, (int)sizeof(T)};
  return HTA_OK;
}

}  // namespace hta

extern "C" {

int hta_hmc_gaussian_forget(void* workspace) {
  std::lock_guard<std::mutex> lock(hta::g_eig_mu);
  for (auto it = hta::g_eig_prepared.begin(); it != hta::g_eig_prepared.end();)
    it = (it->first.first == hta::eig_device() && it->second.base == workspace) ? hta::g_eig_prepared.erase(it) : std::next(it);
  return HTA_OK;
}

int64_t hta_hmc_gaussian_workspace_bytes(int64_t C, int D, int n_traj, int elem_size) {
  if (D > 6)      /* wave-per-chain kernels draw inline: only the eig area V | Vt | lam of the eigenbasis route (+ the slab of its one
                     diagonalisation where D x D does not fit one CU's LDS twice: fp64 from D = 100) */
    return hta::wave_eig_area_bytes(D, elem_size) + (D <= 128 ? hta::metric_eval_workspace_bytes(1, D, elem_size) : 0);
  const int per_vec = 16 / elem_size;
  const int64_t rec = ((int64_t)(D + 1 + per_vec - 1) / per_vec) * per_vec;
  /* + four rows read ahead by the last trajectories, + the eigen block (lam, Qt, Tin, Tout; D <= 6) of the eigenbasis route */
  return ((int64_t)n_traj + hta::QUAD_SLOTS_MAX) * C * rec * elem_size + (D <= 6 ? hta::EIG_ELEMS * elem_size : 0);
}

int64_t hta_hmc_gaussian_status_offset(int64_t C, int D, int n_traj, int elem_size) {
  if (D < 1 || D > 4 || elem_size != 4 || C <= 0 || n_traj < 0) return -1;                /* the fused quad route: fp32, D <= 4 */
  return hta_hmc_gaussian_workspace_bytes(C, D, n_traj, elem_size) - hta::EIG_ELEMS * elem_size + hta::QUAD_STATUS_OFF * 4;
}

#define HTA_DEFINE_GAUSS(SUF, T)                                                                               \
  int hta_hmc_gaussian_sample_##SUF(T* theta, const T* theta_init, const T* P, const T* mu, T log_norm,         \
                                    int mass_kind, const T* inv_mass, const T* mass_factor, int64_t C, int D,   \
                                    int L, T eps, int n_traj, int traj_offset, int burn, uint64_t seed,         \
                                    uint64_t chain_offset, T* samples, int32_t* reject_count, T* H_old,         \
                                    T* H_new, uint8_t* accept, void* workspace, int64_t workspace_bytes,        \
                                    void* stream) {                                                             \
    hta::GaussArgs<T> a{theta, theta_init, P, mu, log_norm, inv_mass, mass_factor, C, D, L, eps, n_traj,         \
                        traj_offset, burn, seed, chain_offset, samples, reject_count, H_old, H_new, accept,     \
                        nullptr, nullptr, nullptr, nullptr, nullptr};                                           \
    const int64_t need = hta_hmc_gaussian_workspace_bytes(C, D, n_traj, (int)sizeof(T));                       \
    if (workspace && workspace_bytes >= need && need > 0) {                                                     \
      a.ws_z = D <= 6 ? (T*)workspace : nullptr;                                                                \
      a.ws_logu = D <= 6 ? (T*)((char*)workspace + need) - hta::EIG_ELEMS : (T*)workspace;  /* eig block / eig area */     \
    }                                                                                                           \
    return hta::gaussian_dispatch<T>(a, mass_kind, false, (hipStream_t)stream);                                 \
  }                                                                                                             \
  int hta_hmc_gaussian_leapfrog_##SUF(T* theta, T* p, const T* P, const T* mu, int mass_kind, const T* inv_mass, \
                                      int64_t C, int D, int steps, T eps, T* path_theta, T* path_p,             \
                                      void* stream) {                                                           \
    hta::GaussArgs<T> a{theta, nullptr, P, mu, (T)0, inv_mass, nullptr, C, D, steps, eps, 0, 0, 0, 0, 0,         \
                        nullptr, nullptr, nullptr, nullptr, nullptr, p, path_theta, path_p, nullptr, nullptr};  \
    return hta::gaussian_dispatch<T>(a, mass_kind, true, (hipStream_t)stream);                                  \
  }

HTA_DEFINE_GAUSS(f32, float)
HTA_DEFINE_GAUSS(f64, double)

#define HTA_DEFINE_GAUSS_PREP(SUF, T)                                                                           \
  int hta_hmc_gaussian_prepare_##SUF(const T* P, int mass_kind, const T* mass_factor, int64_t C, int D,          \
                                     int n_traj, void* workspace, int64_t workspace_bytes, void* stream) {       \
    const int64_t need = hta_hmc_gaussian_workspace_bytes(C, D, n_traj, (int)sizeof(T));                        \
    return hta::gaussian_prepare<T>(P, mass_kind, mass_factor, C, D, n_traj, workspace, workspace_bytes, need,   \
                                    (hipStream_t)stream);                                                        \
  }
HTA_DEFINE_GAUSS_PREP(f32, float)
HTA_DEFINE_GAUSS_PREP(f64, double)

}  // extern "C"
