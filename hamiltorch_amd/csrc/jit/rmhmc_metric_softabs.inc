// The soft-abs metric of rmhmc_callback.hip.in (HTA_CB_METRIC_SOFTABS: the reference's metric=SOFTABS), as TEXT: the skeleton includes one
// section at a time (#define HTA_RM_PIECE ..., #include HTA_RM_METRIC_INC) into the place that names it.  Text and not functions for the
// reason cb_hmc_bodies.inc gives: the machine code must not move - and it does with as little as the PLACE of a declaration (a.alpha
// converted after a.jitter, the state arrays declared before th: other registers and spills), which is why a section declares what it
// computes where the kernel always declared it (profiles/r13a_rmhmc_skeleton_code_objects.txt).
//
//   fisher         cyclic Jacobi on the packed symmetric matrix in registers (every index a compile-time constant: the sweeps are fully
//                  unrolled; lanes run the same rotation schedule, a wave leaves the sweep loop when all its lanes have converged),
//                  soft-abs map (S:120);
//   rm_hamiltonian log|G| = sum log lam~ (S:726), p^T G^-1 p in the eigenbasis (S:729-731);
//   gibbs          G = Q lam~ Q^T, its Cholesky factor, p = L z (S:183-184);
//   dH/dp, dH/dth  G^-1 m in the eigenbasis; -(grad + c), c_k = <d_k Hess, M>, M = Q W Q^T the Daleckii-Krein form of the soft-abs
//                  derivative (oracle.softabs_dmetric; csrc/rmhmc_metric.hip computes the same M for larger systems).
//
// DEFS (namespace hta_cb): the kernel's name and set, HTA_RM_PARAMS (a.alpha), the array the momentum draw goes through, the
//   eigensolver and the slope of the map.
// STATE: what an evaluation leaves for the next ops - eigenvalues, their soft-abs images, eigenvectors (the next warm start).
// FACTOR: A (-Hessian + jitter, packed; destroyed) into the state.  GIBBS: T G[NT], the Cholesky factor of G (HTA_RM_GIBBS_L).
// SOLVE: u (G^-1 m = Q u), T quad = m^T G^-1 m and T logdet, in every mode.  LOGDET, BACKSOLVE: nothing here.
// DRIFT: delta = eps/2 G^-1 m.  KICK_MATRIX: T M[NT].
#if HTA_RM_PIECE == HTA_RM_PIECE_DEFS
#define HTA_RM_KERNEL hta_cb_rmhmc_kernel
#define HTA_RM_SET HTA_CB_SET_RMHMC
#define HTA_RM_GIBBS_L G
#define HTA_RM_PARAMS const T alpha = (T)a.alpha;

constexpr int MAX_SWEEPS = sizeof(T) == 4 ? 14 : 20;
#ifndef HTA_CB_JTOL32
#define HTA_CB_JTOL32 1e-10      // float: |off| / |diag| <= 1e-5 (eigenvalues to ~1e-10 relative, vectors to ~1e-5 / relative gap)
#endif

// 1 ulp hardware forms for the rotation angles of the Jacobi sweeps (float); double keeps the library forms
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ double fast_rcp(double x) { return 1.0 / x; }
__device__ __forceinline__ float fast_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ double fast_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float fast_rsqrt(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ double fast_rsqrt(double x) { return 1.0 / sqrt(x); }

// Cyclic Jacobi on the packed symmetric A (destroyed: its diagonal ends as the eigenvalues); V = eigenvectors in columns, V[i * D + k].
// warm: V holds the eigenvectors of the PREVIOUS evaluation of this trajectory (a nearby matrix: the same point with another jitter
// draw, or half a step away) - A is first rotated into that basis (B = V^T A V: 2 D^3 multiply-adds), where it is nearly diagonal, so
// two or three sweeps finish it instead of seven or eight from the identity; the rotations then continue on V.  The first evaluation of
// every trajectory starts cold, which also bounds the drift of V^T V - I (as rmhmc._WarmBases.reset does for the launch sequence).
__device__ __forceinline__ void jacobi_eig(T (&A)[NT], T (&V)[D * D], bool warm) {
  if (warm) {
    T B[NT];
#pragma unroll
    for (int l = 0; l < D; ++l) {
      T t[D];                                                      // column l of A V
#pragma unroll
      for (int i = 0; i < D; ++i) {
        T s = 0;
#pragma unroll
        for (int j = 0; j < D; ++j) s += A[tri(i, j)] * V[j * D + l];
        t[i] = s;
      }
#pragma unroll
      for (int k = l; k < D; ++k) {
        T s = 0;
#pragma unroll
        for (int i = 0; i < D; ++i) s += V[i * D + k] * t[i];
        B[tri(k, l)] = s;
      }
    }
#pragma unroll
    for (int e = 0; e < NT; ++e) A[e] = B[e];
  } else {
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int k = 0; k < D; ++k) V[i * D + k] = (i == k) ? (T)1 : (T)0;
  }
  // on the squared off-diagonal mass relative to the squared diagonal: |off| / |diag| <= 2e-6 (float) / 1e-13 (double) - a few D eps,
  // the floor the rotations' own rounding leaves (a tighter bound is never met in float32 and every call runs all MAX_SWEEPS)
  const T tol = sizeof(T) == 4 ? (T)HTA_CB_JTOL32 : (T)1e-26;
  for (int sweep = 0; sweep < MAX_SWEEPS; ++sweep) {
    T off = 0, dg = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      dg += A[tri(i, i)] * A[tri(i, i)];
#pragma unroll
      for (int j = 0; j < i; ++j) off += A[tri(i, j)] * A[tri(i, j)];
    }
    // (a lane with non-finite entries never converges: the sweep limit ends the loop, the energies come out non-finite, the proposal
    //  is rejected - the LogProbError path of S:110-112)
    const bool busy = !(off <= tol * dg) && (off == off) && (dg == dg) && !cb_isinf(off + dg);
    if (!__any(busy)) break;
    // threshold Jacobi: an element whose square is below its share of the stopping bound is left alone - and when that holds in
    // EVERY lane of the wave the rotation is skipped altogether (after a warm start most of the 55 are)
    const T thr2 = tol * dg * (T)(0.5 / NT);
#pragma unroll
    for (int p = 0; p < D - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < D; ++q) {
        const T apq = A[tri(q, p)];
        const bool rot = apq * apq > thr2;
        if (!__any(rot)) continue;
        const T app = A[tri(p, p)], aqq = A[tri(q, q)];
        // tan of the rotation angle, the smaller root: t = sgn(th) / (|th| + sqrt(th^2 + 1)), th = (aqq - app) / (2 apq).
        // (c, s) only have to be A rotation close to that angle (the iteration corrects itself, V stays orthogonal to rounding as long
        // as c^2 + s^2 = 1 to rounding): float uses the hardware reciprocal / square root / reciprocal square root (1 ulp) instead of
        // the correctly rounded divisions (~10 instructions each)
        const T th = (aqq - app) * fast_rcp((T)2 * (rot ? apq : (T)1));
        const T tt = (th >= (T)0 ? (T)1 : (T)-1) * fast_rcp(cb_abs(th) + fast_sqrt(th * th + (T)1));
        const T t = rot ? tt : (T)0;
        const T c = fast_rsqrt(t * t + (T)1), s = t * c;
        A[tri(p, p)] = app - t * apq;
        A[tri(q, q)] = aqq + t * apq;
        A[tri(q, p)] = rot ? (T)0 : apq;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          if (k != p && k != q) {
            const T akp = A[tri(k, p)], akq = A[tri(k, q)];
            A[tri(k, p)] = c * akp - s * akq;
            A[tri(k, q)] = s * akp + c * akq;
          }
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const T vkp = V[k * D + p], vkq = V[k * D + q];
          V[k * D + p] = c * vkp - s * vkq;
          V[k * D + q] = s * vkp + c * vkq;
        }
      }
    }
  }
}

// d lam~ / d lam of lam~ = lam coth(alpha lam)  (csrc/rmhmc_metric_dev.hpp: softabs_slope)
__device__ __forceinline__ T softabs_slope(T alpha, T lam) {
  const T x = alpha * lam, ax = cb_abs(x);
  const T x2 = x * x;
  const T ser = x * ((T)(2.0 / 3.0) - x2 * ((T)(4.0 / 45.0) - x2 * ((T)(12.0 / 945.0) - x2 * (T)(8.0 / 4725.0))));
  const T t = cb_exp((T)-2 * ax), om = (T)1 - t;
  const T d = ((T)1 + t) / om - ax * (T)4 * t / (om * om);
  return ax < (T)0.3 ? ser : (x < 0 ? -d : d);
}

#elif HTA_RM_PIECE == HTA_RM_PIECE_STATE
  T lam[D], lt[D], V[D * D];

#elif HTA_RM_PIECE == HTA_RM_PIECE_FACTOR
        jacobi_eig(A, V, op != 0);
#pragma unroll
        for (int i = 0; i < D; ++i) {
          lam[i] = A[tri(i, i)];
          lt[i] = ((T)1 / cb_tanh(alpha * lam[i])) * lam[i];          // S:120
        }

#elif HTA_RM_PIECE == HTA_RM_PIECE_GIBBS
        // G = Q diag(lam~) Q^T (S:121) and its Cholesky factor
        T G[NT];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j) {
            T s = 0;
#pragma unroll
            for (int q = 0; q < D; ++q) s += V[i * D + q] * lt[q] * V[j * D + q];
            G[tri(i, j)] = s;
          }
#pragma unroll
        for (int j = 0; j < D; ++j) {
          T d = G[tri(j, j)];
#pragma unroll
          for (int q = 0; q < j; ++q) d -= G[tri(j, q)] * G[tri(j, q)];
          d = cb_sqrt(d);
          G[tri(j, j)] = d;
#pragma unroll
          for (int i = j + 1; i < D; ++i) {
            T s = G[tri(i, j)];
#pragma unroll
            for (int q = 0; q < j; ++q) s -= G[tri(i, q)] * G[tri(j, q)];
            G[tri(i, j)] = s / d;                                     // (a division: not the reciprocal form of the Metric.HESSIAN factor)
          }
        }

#elif HTA_RM_PIECE == HTA_RM_PIECE_SOLVE
      // ---- u = Q^T m / lam~;  G^-1 m = Q u;  m^T G^-1 m = sum w u
      T u[D];
      T quad = 0, logdet = 0;
#pragma unroll
      for (int q = 0; q < D; ++q) {
        T w = 0;
#pragma unroll
        for (int i = 0; i < D; ++i) w += V[i * D + q] * m[i];
        u[q] = w / lt[q];
        quad += w * u[q];
        logdet += cb_log(lt[q]);                                      // S:726 (in every mode)
      }

#elif HTA_RM_PIECE == HTA_RM_PIECE_LOGDET || HTA_RM_PIECE == HTA_RM_PIECE_BACKSOLVE

#elif HTA_RM_PIECE == HTA_RM_PIECE_DRIFT
#pragma unroll
        for (int i = 0; i < D; ++i) {
          T s = 0;
#pragma unroll
          for (int q = 0; q < D; ++q) s += V[i * D + q] * u[q];
          delta[i] = eh * s;
        }

#elif HTA_RM_PIECE == HTA_RM_PIECE_KICK_MATRIX
        // M = Q W Q^T, W_kl = 1/2 [k == l] lam~'_k / lam~_k - 1/2 J_kl u_k u_l, J the divided difference of the soft-abs map (S:395-398)
        T W[NT], slope[D];
        const T tol = sizeof(T) == 4 ? (T)1e-3 : (T)1e-6;
#pragma unroll
        for (int q = 0; q < D; ++q) slope[q] = softabs_slope(alpha, lam[q]);
#pragma unroll
        for (int q = 0; q < D; ++q)
#pragma unroll
          for (int l = 0; l <= q; ++l) {
            const T dl = lam[q] - lam[l];
            const bool close = (q == l) || cb_abs(dl) <= tol * (cb_abs(lam[q]) + cb_abs(lam[l]));
            // (the slope at the midpoint - an exp and two divisions - only where some lane of the wave has a coinciding pair)
            T J = (lt[q] - lt[l]) / (close ? (T)1 : dl);
            if (q == l) J = slope[q];
            else if (__any(close)) J = close ? softabs_slope(alpha, (T)0.5 * (lam[q] + lam[l])) : J;
            T w = (T)-0.5 * J * u[q] * u[l];
            if (q == l) w += (T)0.5 * slope[q] / lt[q];
            W[tri(q, l)] = w;
          }
        T M[NT];
#pragma unroll
        for (int i = 0; i < D; ++i) {
          T row[D];                                                   // row i of Q W
#pragma unroll
          for (int l = 0; l < D; ++l) {
            T s = 0;
#pragma unroll
            for (int q = 0; q < D; ++q) s += V[i * D + q] * W[tri(q, l)];
            row[l] = s;
          }
#pragma unroll
          for (int j = 0; j <= i; ++j) {
            T s = 0;
#pragma unroll
            for (int l = 0; l < D; ++l) s += row[l] * V[j * D + l];
            M[tri(i, j)] = s;
          }
        }

#else
#error "rmhmc_metric_softabs.inc: define HTA_RM_PIECE"
#endif
#undef HTA_RM_PIECE
