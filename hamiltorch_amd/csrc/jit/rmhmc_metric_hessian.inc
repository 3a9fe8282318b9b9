// Metric.HESSIAN of rmhmc_callback.hip.in (HTA_CB_METRIC_HESSIAN), as TEXT in the sections of rmhmc_metric_softabs.inc.
//
// The reference's default metric (hamiltorch/samplers.py, sample(..., metric=Metric.HESSIAN), S:850) is G = -Hessian(log p) itself
// (S:108-117): the Girolami-Calderhead form for log-concave posteriors.
//
//   fisher         the packed Cholesky factor G = L L^T IN PLACE (every index a compile-time constant).  No eigendecomposition, no
//                  basis: L (and 1 / L_ii) is all that persists between ops.  A pivot that is not positive gives NaN through plain
//                  arithmetic (sqrt of a negative number; 1 / 0) - where the reference's `cholesky` raises (S:146), and what
//                  csrc/rmhmc_metric_mfma.hip does: the energies come out non-finite, mh_accept rejects;
//   gibbs          p = L z (S:183-184) with the factor itself;
//   rm_hamiltonian y = L^-1 m, m^T G^-1 m = y^T y, log|G| = 2 sum log L_ii (= slogdet of S:728 for a positive definite G);
//   dH/dp          v = L^-T y (S:146-148);
//   dH/dth         -(grad + c), c_k = <d_k Hess, M>, M = 1/2 G^-1 - 1/2 v v^T (oracle.hessian_dmetric), G^-1 = L^-T L^-1 packed.
//
// a.alpha is not read.  One chain per lane, no LDS, no barrier, no cross-lane operation.
//
// DEFS: the kernel's name and set, HTA_RM_PARAMS (none), `cholesky`.  STATE: the factor and 1 / its diagonal.  FACTOR: A into the
// state.  GIBBS: nothing - the draw goes through Lf (HTA_RM_GIBBS_L).  SOLVE: y, T quad.  LOGDET (under ENERGY only): T logdet.
// BACKSOLVE: v = G^-1 m (DRIFT and KICK_MATRIX read it).  DRIFT: delta = eps/2 v.  KICK_MATRIX: T M[NT].
#if HTA_RM_PIECE == HTA_RM_PIECE_DEFS
#define HTA_RM_KERNEL hta_cb_rmhmc_hess_kernel
#define HTA_RM_SET HTA_CB_SET_RMHMC_HESS
#define HTA_RM_GIBBS_L Lf
#define HTA_RM_PARAMS

// G = L L^T in place on the packed lower triangle; rd[i] = 1 / L_ii.  No test of the pivot: a negative one is a NaN from the square
// root on, a zero one an infinite rd - either way every later product of this evaluation is non-finite.
__device__ __forceinline__ void cholesky(T (&A)[NT], T (&rd)[D]) {
#pragma unroll
  for (int j = 0; j < D; ++j) {
    T d = A[tri(j, j)];
#pragma unroll
    for (int q = 0; q < j; ++q) d -= A[tri(j, q)] * A[tri(j, q)];
    d = cb_sqrt(d);
    const T r = (T)1 / d;
    A[tri(j, j)] = d;
    rd[j] = r;
#pragma unroll
    for (int i = j + 1; i < D; ++i) {
      T s = A[tri(i, j)];
#pragma unroll
      for (int q = 0; q < j; ++q) s -= A[tri(i, q)] * A[tri(j, q)];
      A[tri(i, j)] = s * r;                                           // (the stored reciprocal: not the division of the soft-abs draw)
    }
  }
}

#elif HTA_RM_PIECE == HTA_RM_PIECE_STATE
  T Lf[NT], rd[D];

#elif HTA_RM_PIECE == HTA_RM_PIECE_FACTOR
        cholesky(A, rd);
#pragma unroll
        for (int e = 0; e < NT; ++e) Lf[e] = A[e];

#elif HTA_RM_PIECE == HTA_RM_PIECE_GIBBS

#elif HTA_RM_PIECE == HTA_RM_PIECE_SOLVE
      // ---- y = L^-1 m;  m^T G^-1 m = y^T y
      T y[D];
      T quad = 0;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        T s = m[i];
#pragma unroll
        for (int q = 0; q < i; ++q) s -= Lf[tri(i, q)] * y[q];
        y[i] = s * rd[i];
        quad += y[i] * y[i];
      }

#elif HTA_RM_PIECE == HTA_RM_PIECE_LOGDET
        T logdet = 0;
#pragma unroll
        for (int i = 0; i < D; ++i) logdet += cb_log(Lf[tri(i, i)]);
        logdet *= (T)2;                                               // S:728

#elif HTA_RM_PIECE == HTA_RM_PIECE_BACKSOLVE
      // ---- v = G^-1 m = L^-T y (S:146-148)
      T v[D];
#pragma unroll
      for (int i = D - 1; i >= 0; --i) {
        T s = y[i];
#pragma unroll
        for (int q = i + 1; q < D; ++q) s -= Lf[tri(q, i)] * v[q];
        v[i] = s * rd[i];
      }

#elif HTA_RM_PIECE == HTA_RM_PIECE_DRIFT
#pragma unroll
        for (int i = 0; i < D; ++i) delta[i] = eh * v[i];

#elif HTA_RM_PIECE == HTA_RM_PIECE_KICK_MATRIX
        // M = 1/2 G^-1 - 1/2 v v^T (S:395-398 through the Cholesky factor)
        T W[NT];                                                      // L^-1, column by column
#pragma unroll
        for (int j = 0; j < D; ++j) {
          W[tri(j, j)] = rd[j];
#pragma unroll
          for (int i = j + 1; i < D; ++i) {
            T s = 0;
#pragma unroll
            for (int q = j; q < i; ++q) s -= Lf[tri(i, q)] * W[tri(q, j)];
            W[tri(i, j)] = s * rd[i];
          }
        }
        T M[NT];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j) {
            T s = 0;                                                  // (G^-1)_ij = sum_{q >= i} (L^-1)_qi (L^-1)_qj
#pragma unroll
            for (int q = i; q < D; ++q) s += W[tri(q, i)] * W[tri(q, j)];
            M[tri(i, j)] = (T)0.5 * s - (T)0.5 * v[i] * v[j];
          }

#else
#error "rmhmc_metric_hessian.inc: define HTA_RM_PIECE"
#endif
#undef HTA_RM_PIECE
