#define HTA_PHILOX_MAD64 1      // philox.hpp: 64-bit products (this file's kernels have the registers for them)
// Riemannian-metric evaluation on the matrix cores (fp32, D <= 112): the evaluations of a constant-curvature target, which
// all start from ONE shared eigenbasis.
//
// Same contract as metric_eval_kernel (rmhmc_metric.hip): per system b it replaces
//   fisher()            (samplers.py:108-122)  Hs + jitter*U(0,1) on the diagonal -> eigh -> lam/tanh(alpha lam) -> Q diag Q^T
//   cholesky_inverse()  (samplers.py:146-148)  G^-1 p
//   rm_hamiltonian()    (samplers.py:710-731)  -logp + D/2 log 2pi + 1/2 log|G| + 1/2 p^T G^-1 p
//   gibbs(RMHMC)        (samplers.py:183-184)  p = chol(G) z
// and the fused first-order updates of an explicit half step (samplers.py:429-458).
//
// The eigendecomposition.  Every evaluation's matrix is Hs_b = P + diag(e_b), e_b = jitter * U(0,1)^D (S:113-115), and the
// driver has diagonalised the jitter-free P once (V0, lam0).  In that basis A = V0^T Hs_b V0 = diag(lam0) + V0^T diag(e) V0
// is a small perturbation of a diagonal matrix, and its eigenvectors are REFINED from X = I by the iteration of Ogita &
// Aishima (Japan J. Indust. Appl. Math. 35, 2018: "Iterative refinement for symmetric eigenvalue decomposition"):
//     S = X^T A X,  Gm = X^T X,  lam_i = S_ii / Gm_ii,
//     E_ii = (1 - Gm_ii) / 2,   E_ij = (S_ij - lam_j Gm_ij) / (lam_j - lam_i),   X <- X (I + E),
// quadratically convergent, and nothing but dense products (formation of A, A X, X^T (A X), X^T X, X E) as
// v_mfma_f32_16x16x4_f32 tiles (exact fp32 products, fp32 accumulation) on [DP][LD] buffers in LDS.  The
// iteration needs the coupling to be small against the eigenvalue gaps; max |E_ij| says whether it is: above 0.03 (a
// nearly degenerate spectrum, a large jitter, a stalled iteration) the system falls back - inside the same launch - to
// the cyclic Jacobi solver of rmhmc_metric.hip, which needs no such assumption.  Results agree with that solver to
// rounding (tests/test_gpu_rmhmc.py::test_metric_mfma_kernel_equals_jacobi_kernel); hta_set_tuning("metric_mfma", 0)
// selects it outright.
// Round 4: the first pass starts from X = I, so X = I + E1 with E1 antisymmetric; where max |E1_ij| <= 8e-3 (BASELINE config 3:
// 5e-3) the SECOND pass is taken in closed form - second-order perturbation theory, ONE product F E1 (ph_refine_E2) instead of
// A X, X^T A X and X^T X - and applied to the vectors of a solve without being formed: two D^3 products per solve evaluation
// (formation, F E1); hta_set_tuning("metric_second", 0) keeps the three-product pass.  And a TRAJECTORY of the Gaussian-target
// sampler is one launch (metric_traj_mfma_kernel below): the chain's workgroup runs its 4 L + 3 evaluations back to back.
//
// Round 6: the SOLVE evaluations of a Gaussian target on the shared basis - 4 L + 2 of a trajectory's 4 L + 3 - and, by default, its momentum
// draw (p = G^(1/2) z, solve-shaped) run a reorganised sequence of the same mathematics (metric_fast_solve and the ph_fast_* phases, rmhmc_metric_mfma_fast_dev.hpp: V0
// resident, the element-wise passes in the products' epilogues, the second-order product as three bfloat16 products on pre-split operands,
// vector phases on 8 waves, the trajectory's state resident in LDS in eigen-coordinates): 35 k cycles per evaluation instead of 71 k.  What
// follows in this header describes the GENERAL sequence (metric_warm_system), which still serves everything else: per-system curvature and
// bases, outputs that need G or Q, Metric.HESSIAN, and whatever the fast sequence declines.
//
// The momentum draw / fisher() outputs add Q = V0 X, G = Q diag(lam~) Q^T (two more GEMMs) and a right-looking Cholesky in
// 16-column panels whose triangular solve and trailing update are MFMA tiles as well.
// Matrix-vector products (V0^T m, X^T m', X w, V0 x', P d) use all 1024 threads: 8 lanes per row, DPP-free shuffles.
//
// One translation unit in layers.  This file: the tuning keys, the two kernels, the eligibility predicates and the host launchers.  The device
// code, bottom up: ..._gemm_dev.hpp (the MFMA products), ..._vec_dev.hpp (DPP reductions, matrix-vector products, the panel Cholesky),
// ..._phases_dev.hpp (the general sequence's out-of-line phases), ..._fast_dev.hpp (the LDS layout, the fast solve, the resident state),
// ..._general_dev.hpp (metric_warm_system, the out-of-line evaluations of the kernels, the Metropolis selection).
#include "rmhmc.hpp"
#include "rmhmc_metric_mfma_gemm_dev.hpp"
#include "rmhmc_metric_mfma_vec_dev.hpp"
#include "rmhmc_metric_mfma_phases_dev.hpp"
#include "rmhmc_metric_mfma_fast_dev.hpp"
#include "rmhmc_metric_mfma_general_dev.hpp"

namespace hta {

int g_metric_mfma = 1;      // tuning key "metric_mfma": 1 = warm fp32 evaluations run here, 0 = always the Jacobi kernel
int g_metric_second = 1;    // tuning key "metric_second": 1 = the refinement's second pass in closed form (one product: ph_refine_E2) where the first pass's update is small, 0 = always the full pass (three products)
int g_metric_bx3 = 2;       // tuning key "metric_bx3": 2 = the fast solve's formation AND its second-pass product F E1 as three bfloat16 products of operands split hi + lo, 1 = F E1 only (the formation in exact fp32), 0 = exact fp32 products
int g_metric_sqrtdraw = 1;  // tuning key "metric_sqrtdraw": 1 = the momentum draw of soft-abs evaluations on a shared basis is p = G^(1/2) z (the symmetric square root: a SOLVE-shaped
                            // evaluation - same law as S:183-184's chol(G) z, no assembly of G, no Cholesky), 0 = the reference's map chol(G) z
int g_metric_general = 1;   // tuning key "metric_general": 1 = evaluations with per-system curvature AND per-system bases run here too
int g_metric_select = 1;    // tuning key "metric_select": 1 = the trajectory kernel ends with the chain's Metropolis selection (one launch per trajectory), 0 = mh_select is a second launch
int g_metric_resident = 1;  // tuning key "metric_resident": 1 = the trajectory kernel keeps the chain's state in LDS in eigen-coordinates, 0 = in the caller's (bit-identical to the launch sequence)
int g_metric_traj = 1;      // tuning key "metric_traj": 1 = a trajectory of the eigendecomposition route is one launch, 0 = one launch per evaluation

// One evaluation per system: the fast solve where it applies, else the general sequence - out of line (warm_general_eval), so that the kernel's
// own body keeps only what the fast solve reads.
__global__ __launch_bounds__(MT) void metric_warm_mfma_kernel(MetricArgsT<float> a, int DP, int LD, int second) {
  const int tiles = fast_tiles(DP / 16);
  const kernarg_ptr ka = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
  // what metric_warm_system's own hook tests, evaluated once per launch: the fast solve covers solves and solve-shaped draws of a soft-abs
  // metric on a shared basis
  const bool softabs = a.metric == 1, general = softabs && a.hs_stride != 0;
  const bool sdraw = (second & kSecSqrtDraw) && a.p_out && softabs && !general && !a.m && !a.G_out && !a.V_out && !a.dmetric_out;
  const bool fast = (second & kSecClosed) && softabs && !general && (a.m || sdraw) && !(a.G_out || (a.p_out && !sdraw) || a.V_out || a.dmetric_out) &&
                    (!a.X || a.Pm == a.Hs);
  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    int vres = -1;
    if (fast && metric_fast_solve(a, DP, LD, b, vres, (second & kSecBf16) != 0, tiles, -1, 0, sdraw, (second & kSecBf16Form) != 0)) continue;
    warm_general_eval(ka, DP, LD, b, vres, second | kSecFastDeclined, tiles);
  }
}

__global__ __launch_bounds__(MT) void metric_traj_mfma_kernel(MetricArgsT<float> a, MetricTrajArgs t, int DP, int LD, int second) {
  const int D = a.D;
  const int nops = 4 * t.L + 3;
  const int tiles = fast_tiles(DP / 16);
  const kernarg_ptr ka = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
  // RESIDENT mode (round 6, kSecResident: tuning key "metric_resident"): after the momentum draw the chain's four state vectors are taken
  // into the eigenbasis ONCE - theta' = V0^T (theta - mu), p' = V0^T p - and live in LDS for the trajectory: a solve evaluation then has
  // no V0 product at either end (m' and d' ARE the state, x' and lam0 d' update it element-wise), no global read or write but its
  // scalars; the binding rotation is element-wise in any orthonormal basis.  theta = mu + V0 theta' once at the end.  The rounding of
  // the 4 L + 2 round trips through V0 is gone, not added: results agree with the launch sequence to fp32 rounding, not bit for bit
  // (without kSecResident the form is bit-identical: tests/test_gpu_rmhmc.py::test_trajectory_kernel_equals_the_launch_sequence).
  const bool resident = (second & kSecResident) && (second & kSecClosed) && a.metric == 1 && a.hs_stride == 0 && a.Pm == a.Hs && a.V0 && a.lam0;
  const TrajLds lay(DP, LD);
  const int BS = lay.BS, oY = lay.oY, sTh = lay.sTh, sP = lay.sP, sThc = lay.sThc, sPc = lay.sPc;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* const lds0 = reinterpret_cast<float*>(smem_raw);
  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    int vres = -1;                       // the buffer a solve left the staged V0 in: the next evaluation starts from it
    if (!resident) {
      for (int op = 0; op < nops; ++op) vres = traj_general_eval(ka, DP, LD, b, vres, op, second, tiles, 0);
      if (t.select) traj_select(a, t, b);
      continue;
    }
    const int64_t e0 = b * D;
    bool drawn = false;
    if (second & kSecSqrtDraw) {
      // the momentum draw p = G^(1/2) z in eigen-coordinates: (theta', z') = V0^T (cur - mu, z) in one pass, then the solve's sequence with
      // m' = z' and w = y sqrt(lam~); its x' IS p' = V0^T p (no way back through V0)
      __syncthreads();
      ph_stage(a.V0, BS, D, DP, LD); vres = BS;
      if ((int)threadIdx.x < DP) {
        const int i = opaque_tid();
        lds0[oY + 2 * i] = i < D ? normal_elem<float>(a.seed, a.chain_offset + (uint64_t)b, a.draw, 0, i) : 0.f;
        lds0[oY + 2 * i + 1] = i < D ? t.cur[e0 + i] - a.mu[i] : 0.f;
      }
      __syncthreads();
      ph_fast_vt(vres, oY, sP, sTh, DP, LD);
      MetricArgsT<float> o = a;
      o.sub = 0; o.X = nullptr; o.m = nullptr; o.p_out = t.pm;
      drawn = metric_fast_solve(o, DP, LD, b, vres, (second & kSecBf16) != 0, tiles, (sTh >> 2) | ((sP >> 2) << 16), sP >> 2, true, (second & kSecBf16Form) != 0);
    }
    if (!drawn) {
      vres = traj_general_eval(ka, DP, LD, b, vres, 0, second, tiles, 0);                      // the draw on the general sequence (p in t.pm)
      // into the eigenbasis: (theta', p') = V0^T (cur - mu, pm)
      __syncthreads();
      if (vres < 0) { ph_stage(a.V0, BS, D, DP, LD); vres = BS; }
      res_in(vres, oY, sTh, sP, t.cur + e0, t.pm + e0, a.mu, D, DP, LD);
    }
    __syncthreads();
    if ((int)threadIdx.x < DP) { const int i = opaque_tid(); lds0[sThc + i] = lds0[sTh + i]; lds0[sPc + i] = lds0[sP + i]; }   // theta~' = theta', p~' = p'
    __syncthreads();
    for (int op = 1; op < nops; ++op) {
      // the fields the fast solve reads (everything else of `a` is dead here); the decode of `op` is traj_general_eval's: the two must agree
      MetricArgsT<float> o = a;
      o.X = t.cur; o.m = t.pm;                                                                 // (non-null: the operands themselves are the resident vectors)
      int j = -1;
      bool fa = false;
      if (op == 1) { o.sub = 1; o.H_out = t.H0; }                                              // H_old  S:971
      else if (op == nops - 1) { o.sub = 2u + 8u * (uint32_t)t.L; o.H_out = t.H1; o.logp_out = t.lp1; }   // H_new  S:989
      else {
        const int q = op - 2, l = q >> 2;
        j = q & 3;
        fa = j == 0 || j == 3;                                                                 // phi_A/2 (S:429-430, S:457-458) : phi_B/2
        o.sub = 2u + 8u * (uint32_t)l + (j == 0 ? 1u : j == 1 ? 2u : j == 2 ? 4u : 7u);
        o.cx = t.eh; o.cg = -t.eh;
      }
      const bool step = j >= 0;
      const int rx = (step && !fa) ? sThc : sTh, rm = (step && fa) ? sPc : sP;
      const int upd = step ? (((fa ? sThc : sTh) >> 2) | (((fa ? sP : sPc) >> 2) << 16)) : 0;
      if (!metric_fast_solve(o, DP, LD, b, vres, (second & kSecBf16) != 0, tiles, (rx >> 2) | ((rm >> 2) << 16), upd, false, (second & kSecBf16Form) != 0))
        vres = traj_general_eval(ka, DP, LD, b, vres, op, second | kSecCallerRotates, tiles, 1);                  // (rare: a first pass above kSecondE, a non-finite state)
      if (j == 1) {                                                                            // phi_C  S:447-450 (element-wise: any orthonormal basis)
        __syncthreads();
        const int i = opaque_tid();
        if (i < D) phi_c_elem<float>(lds0[sTh + i], lds0[sP + i], lds0[sThc + i], lds0[sPc + i], t.c, t.s);
      }
    }
    // back: theta = mu + V0 theta' (and the final momentum, as the other form leaves it)
    __syncthreads();
    ph_res_out(vres, sTh, sP, t.th + e0, t.pm + e0, a.mu, D, DP, LD);
    if (t.select) traj_select(a, t, b);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// the kernels' `second` argument from the tuning keys (the trajectory launcher adds kSecResident)
static int metric_second_bits() {
  return (g_metric_second ? kSecClosed : 0) | (g_metric_bx3 ? kSecBf16 : 0) | (g_metric_sqrtdraw ? kSecSqrtDraw : 0) | (g_metric_bx3 >= 2 ? kSecBf16Form : 0);
}

// What both launchers do before the launch: the padded shape and its LDS block (MetricLds) against the CU's 160 KiB, the max_sweeps default,
// the kernel's one-time opt-in to that much dynamic LDS, the grid.  `what` / `entry`: the launcher's names in its error texts.
struct MetricLaunch {
  MetricArgsT<float> k;
  int DP, LD, grid;
  size_t lds;
};
static int metric_launch_prepare(const MetricArgsT<float>& a, const void* kernel, DevOnce& done, const char* what, const char* entry, MetricLaunch& p) {
  p.DP = (a.D + 15) / 16 * 16; p.LD = p.DP + 4;
  p.lds = (size_t)MetricLds(p.DP, p.LD).floats * sizeof(float);
  HTA_REQUIRE(p.lds <= 160 * 1024, "%s: D=%d does not fit the LDS", what, a.D);
  p.k = a;
  if (p.k.max_sweeps <= 0) p.k.max_sweeps = 16;
  if (const int rc = allow_big_lds(done, entry, kernel)) return rc;
  p.grid = (int)(a.B < 65536 ? a.B : 65536);
  return HTA_OK;
}

bool metric_traj_mfma_eligible(const MetricArgsT<float>& a) {
  return g_metric_traj && a.hs_stride == 0 && !a.V_out && !a.dmetric_out && !a.G_out && metric_warm_mfma_eligible(a);
}

int metric_traj_mfma(const MetricArgsT<float>& a, const MetricTrajArgs& t, hipStream_t s) {
  static DevOnce done;
  MetricLaunch p;
  if (int rc = metric_launch_prepare(a, reinterpret_cast<const void*>(&metric_traj_mfma_kernel), done, "hta_rmhmc_gaussian_sample (trajectory kernel)",
                                     "hta_rmhmc_gaussian_sample", p))
    return rc;
  profile_begin(s);
  note_route("metric_traj_mfma_kernel");
  metric_traj_mfma_kernel<<<p.grid, MT, p.lds, s>>>(p.k, t, p.DP, p.LD, metric_second_bits() | (g_metric_resident ? kSecResident : 0));
  profile_end(s);
  HTA_CHECK_LAUNCH("hta_rmhmc_gaussian_sample (trajectory kernel)");
  return HTA_OK;
}

bool metric_warm_mfma_eligible(const MetricArgsT<float>& a) {
  if (!g_metric_mfma || a.D < 1 || a.D > 112 || a.L_out) return false;
  if (a.metric == 1) {
    if (a.hs_stride == 0) return a.V0 && a.lam0 && !a.dmetric_out && !a.V_out;      // soft-abs: evaluations that share an eigenbasis
    // per-system curvature with per-system bases (a general target's chains, each warm-started from its previous evaluation);
    // G_out / p_out together with dmetric_out is not a combination the kernel keeps X for
    return g_metric_general && a.V0 && a.v0_stride != 0 && !(a.dmetric_out && (a.G_out || a.p_out));
  }
  return a.metric == 0 && !a.dmetric_out && !a.V_out;                 // Metric.HESSIAN: Cholesky + solve, any curvature input
}

int metric_warm_mfma(const MetricArgsT<float>& a, hipStream_t s) {
  static DevOnce done;
  MetricLaunch p;
  if (int rc = metric_launch_prepare(a, reinterpret_cast<const void*>(&metric_warm_mfma_kernel), done, "hta_metric_eval (mfma)", "hta_metric_eval", p)) return rc;
  profile_begin(s);
  note_route("metric_warm_mfma_kernel");
  metric_warm_mfma_kernel<<<p.grid, MT, p.lds, s>>>(p.k, p.DP, p.LD, metric_second_bits());
  profile_end(s);
  HTA_CHECK_LAUNCH("hta_metric_eval (mfma)");
  return HTA_OK;
}

}  // namespace hta

