// Explicit RMHMC for a Gaussian target when the soft-abs map is the identity: the whole `sample` loop
// (hamiltorch/samplers.py:969-1026 with the integrator S:425-461) for one chain per workgroup, every
// trajectory of a run in ONE launch.
//
// Why this is the same computation as csrc/rmhmc_explicit.hip + rmhmc_metric.hip.  The target's curvature is one
// matrix P for all chains; an evaluation's metric is G = softabs(F), F = P + diag(e), e = jitter u >= 0 (S:113-121).
// lam coth(alpha lam) = lam (1 + 2 exp(-2 alpha lam) + ...): once alpha lam_min(P) >= 20 the correction is below
// 1e-17 relative, i.e. G == F in fp32 and fp64 (and G = F by definition for Metric.HESSIAN).  Then
//   G^-1 m    = (P + E)^-1 m:  x_0 = S m,  x_{k+1} = x_0 - S (e . x_k)  with the shared S = P^-1; contraction factor
//               rho <= jitter / lam_min(P), so K = O(log eps / log rho) products with ONE shared matrix (3 in fp32 at
//               the BASELINE config-3 numbers) instead of an eigendecomposition per chain and evaluation;
//   log |G|   = log |F| and the momentum draw p = chol(G) z (S:183-184): a Cholesky factorisation of F in LDS,
//               three per trajectory (gibbs, H_old, H_new);
//   dH/dtheta = P (theta - mu)  (constant curvature).
// The host (rmhmc_explicit.hip) takes this path only when those conditions hold; everything else - finite alpha,
// indefinite curvature, rho > 1/4, matrices beyond the LDS - keeps the Jacobi path.  Same Philox sub-streams, same
// update order (sequential phi_C, Q1; un-augmented H_new, Q4; first post-burn rejection resets to params_init, Q2).
//
// Layout: P, S and the Cholesky work matrix in LDS (row stride D|1), the four state vectors and scratch vectors in
// LDS, 256 threads: a matrix-vector product is 2 threads per row; the Cholesky trailing update a 16 x 16 thread tile.
#include <math.h>
#include <type_traits>
#include "common.hpp"
#include "rmhmc.hpp"
#include "rmhmc_fused_chain_dev.hpp"
#include "rmhmc_fused_tiles_dev.hpp"
#include "rmhmc_fused_momentum_dev.hpp"

namespace hta {

// ---- this route's tuning keys (hta_set_tuning; declared in rmhmc.hpp, table and defaults in abi.cpp) ----
int g_rmhmc_fused = 1;           // 0 = per-evaluation Jacobi path, 3 = fused with two chains per workgroup (parity tests)
int g_rmhmc_batch = 1;     // fused RMHMC: 16 chains per workgroup on the matrix cores from 2048 chains on (0 off, 2 always)
int g_rmhmc_momwave = 1;   // fused RMHMC: momentum draws by the wave-per-task kernel (fp32, jitter, D <= 104); 0: workgroup-per-task kernel
int g_rmhmc_mfma4 = 1;     // fused RMHMC: four chains per workgroup on v_mfma_f32_4x4x1_16b (0 off, 1 for lo <= chains < hi, 2 always)
int g_rmhmc_mfma4_lo = 1793, g_rmhmc_mfma4_hi = 2049;   // round 4: up to 7 x CUs chains the two-chain kernel of rmhmc_uvc.hip, two workgroups per CU (1536 chains: 2.25e8 against 1.97e8); before:   // round 2 (tracked products): 544 / 640 / 700 chains 1.40x / 1.37x / 1.38x the one-chain kernel, below 513 rmhmc_uv_kernel; round 1: 3072: 0.87x, 4096: 0.88x the 16-chain kernel (a third workgroup per CU doubles a SIMD's load)
int g_rmhmc_pair = 1;        // four-chain kernels: consecutive half steps share product phases (0: one half step at a time)
int g_rmhmc_overlap = 0;   // fused RMHMC: 1 = momentum draws of the next block of trajectories on a side stream (round 3: off -
                           // run beside the trajectory kernel the draws slow it by a third; serial is 3-8 % faster at every chain count)
int g_rmhmc_momsplit = 1;  // fused RMHMC with jitter: p = chol(P) z1 + sqrt(jitter u) . z2 (exactly N(0, P + diag(jitter u)) like
                           // chol(P + diag(jitter u)) z, without a Cholesky per draw); 0 = the per-draw factorisation
int g_rmhmc_wide = 1;      // tuning key "rmhmc_wide": spill-free one-workgroup-per-CU instances of the one-chain kernel

template <typename T> size_t fused_lds_bytes(int D, int* ld_out, int NC = 1, bool need_w = true) {
  const int ld = D | 1;
  if (ld_out) *ld_out = ld;
  return FusedLds(NC, D, ld, need_w).elems * sizeof(T);
}

// Decides whether the identity-soft-abs path applies (lam0: host copy of the jitter-free eigenvalues) and, if so,
// how many refinement products a solve needs (return value K >= 0; -1: the Jacobi path must be used), log |P|, and
// whether the two log-determinants of a trajectory may use log|P + E| = log|P| + tr(SE) - tr((SE)^2)/2, whose
// truncation error is below D rho^3 / 3 (accepted when that is under a quarter ulp of the Hamiltonian's D/2 log 2 pi).
template <typename T>
int fused_plan(const T* lam0_host, int D, int metric, double alpha, int has_jitter, double jitter, double* logdetP, int* series) {
  if (D > 128 || fused_lds_bytes<T>(D, nullptr) > 150 * 1024) return -1;     // 2 row blocks of 64 lanes, slices of <= 64
  double lmin = lam0_host[0], ld = 0;
  for (int i = 0; i < D; ++i) { lmin = lam0_host[i] < lmin ? (double)lam0_host[i] : lmin; ld += log((double)lam0_host[i]); }
  if (!(lmin > 0.0)) return -1;                                     // not positive definite: soft-abs flips signs
  if (metric == HTA_METRIC_SOFTABS && !(alpha * lmin >= 20.0)) return -1;   // coth(alpha lam) != 1 at working precision
  *logdetP = ld; *series = 1;
  if (!has_jitter) return 0;
  if (!(jitter >= 0.0)) return -1;
  const double rho = jitter / lmin;
  if (rho > 0.25) return -1;
  if (rho == 0.0) return 0;
  const double eps = sizeof(T) == 4 ? 6e-8 : 1.1e-16;
  *series = (D * rho * rho * rho / 3.0) <= 0.25 * eps * (0.5 * D);
  int K = (int)ceil(log(eps * 0.25) / log(rho)) - 1;                // relative error after K refinements: rho^(K+1)
  if (K < 1) K = 1;
  return K > 40 ? -1 : K;
}

// side stream + events of the momentum / trajectory overlap, one set per device, created on first use
struct Overlap { hipStream_t side; hipEvent_t start, ready[2], freed[2]; };
static Overlap* overlap_for_current_device() {
  static Overlap pool[16];
  static bool made[16] = {false};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  if (!made[dev]) {
    Overlap& o = pool[dev];
    if (hipStreamCreateWithFlags(&o.side, hipStreamNonBlocking) != hipSuccess) return nullptr;
    bool ok = hipEventCreateWithFlags(&o.start, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 2 && ok; ++i)
      ok = hipEventCreateWithFlags(&o.ready[i], hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&o.freed[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) return nullptr;
    made[dev] = true;
  }
  return &pool[dev];
}

static int fused_cu_count() {
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cus[dev]) {
    hipDeviceProp_t prop;
    cus[dev] = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
  }
  return cus[dev];
}

static constexpr const char* kEntry = "hta_rmhmc_gaussian_sample";     // the entry point allow_big_lds' error text names

// the one-chain kernels' instance of the register slice: f(std::integral_constant<int, KH>{}) for KH = 8, 16 ... 64
template <typename F> static int with_kh(int KH, F&& f) {
  switch (KH) {
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 24: return f(std::integral_constant<int, 24>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 40: return f(std::integral_constant<int, 40>{});
    case 48: return f(std::integral_constant<int, 48>{});
    case 56: return f(std::integral_constant<int, 56>{});
    default: return f(std::integral_constant<int, 64>{});
  }
}

// The code object lists the kernels in the order in which the compiler meets their instances below.  That order is part of what is
// compared byte for byte with the previous code object, so: the row-tile and wide kernels are named inside callables local to this
// function with a declared return type (instantiated, kernels and all, with the function itself), the one-chain kernels under with_kh
// (instantiated at the end of the translation unit), and a callable names the one-chain kernel before the two-chain one.
template <typename T>
int rmhmc_fused_sample(T* cur, const T* theta_init, const T* P, const T* Sinv, const T* mu, double log_norm, double logdetP,
                       int has_jitter, double jitter, int K, int series, int64_t C, int D, int L, double eps, double omega,
                       int n_traj, int traj_offset, int burn, uint64_t seed, uint64_t chain_offset, T* samples,
                       int32_t* reject_count, T* H_old, T* H_new, uint8_t* accept, T* p_ws, int64_t p_ws_elems, const T* LP,
                       hipStream_t s) {
  int ld;
  (void)fused_lds_bytes<T>(D, &ld);
  const float ang = (float)(2.0 * omega * eps);                      // S:435-436: float32 cos / sin whatever the state dtype
  const int grid = (int)(C < 8192 ? C : 8192);
  const int KH = (((D + 1) / 2) + 7) / 8 * 8;                        // register slice: half the contraction range, in eights
  const char* const tname = sizeof(T) == 4 ? "float" : "double";
  // momenta of a block of trajectories are drawn ahead by rmhmc_momentum_kernel when the workspace has room for them.
  // (Through the C ABI it always has: rmhmc_explicit.hip hands over room for at least four trajectories, lending the augmented-state
  //  area if need be, so block > 0 there and the kernels' own draw - fused_body's `else if (NC == 1)` arm - is never asked for.)
  const int64_t per_traj = C * (int64_t)D;
  int block = (p_ws && p_ws_elems >= per_traj) ? (int)(p_ws_elems / per_traj < n_traj ? p_ws_elems / per_traj : n_traj) : 0;
  // With room for two blocks the draws of block b+1 (side stream) overlap the trajectories of block b: the momentum kernel
  // is a quarter of the serial time at config 3, and both kernels are latency bound, so they share the CUs well.
  // p_ws is used as two halves; events order "half drawn" -> trajectories and "half consumed" -> next draw.
  Overlap* ov = nullptr;
  // (from 4096 chains on both kernels fill the chip by themselves and the overlap only makes them contend: 4096 chains
  //  50.5 ms overlapped, 46.6 ms serial; 2048 chains 30.7 ms overlapped, 32.3 ms serial)
  if (g_rmhmc_overlap && block >= 16 && n_traj >= 32 && (C < 4096 || g_rmhmc_overlap == 2)) {
    ov = overlap_for_current_device();
    if (ov) {
      int sub = (n_traj + 7) / 8;                      // ~8 blocks: only the first draw is exposed
      if (sub < 8) sub = 8;
      if (sub > block / 2) sub = block / 2;
      block = sub;
      (void)hipEventRecord(ov->start, s);
      (void)hipStreamWaitEvent(ov->side, ov->start, 0);
    }
  }
  // pre-drawn momenta and no Cholesky inside the trajectory kernel: what every kernel but the one-chain one needs
  const bool lean = block > 0 && (series || !has_jitter);
  // the schedule of a kernel instance: f(std::bool_constant<TRACK>{}), the tracked products with "rmhmc_pair" - fp32 only (the fp64
  // instances would spill twice as much under the 256-register cap, and are not built)
  auto with_track = [&](auto&& f) -> int {
    if constexpr (sizeof(T) == 4) {
      if (g_rmhmc_pair) return f(std::true_type{});
    }
    return f(std::false_type{});
  };
  // which kernel draws a block's momenta
  enum class Draw { split, wave, workgroup };
  const Draw draw = (LP && has_jitter && g_rmhmc_momsplit && D <= 128) ? Draw::split       // p = chol(P) z1 + sqrt(e) . z2: no factorisation per draw
                    : (sizeof(T) == 4 && g_rmhmc_momwave && has_jitter && D <= 104) ? Draw::wave   // fp32, a factorisation per task on one wave, work matrix in registers
                                                                                  : Draw::workgroup;
  int bidx = 0;
  for (int t0 = 0; t0 < n_traj; t0 += (block > 0 ? block : n_traj), ++bidx) {
    const int nt = block > 0 ? (n_traj - t0 < block ? n_traj - t0 : block) : n_traj;
    T* const p_blk = (ov && (bidx & 1)) ? p_ws + (int64_t)block * per_traj : p_ws;
    if (block > 0) {
      static DevOnce done_mom, done_split;     // per T instantiation
      if (draw == Draw::workgroup) { if (const int rc = allow_big_lds(done_mom, kEntry, &rmhmc_momentum_kernel<T>)) return rc; }
      if (draw == Draw::split) { if (const int rc = allow_big_lds(done_split, kEntry, &rmhmc_momentum_split_kernel<T>)) return rc; }
      const int64_t ntask = (int64_t)nt * C;
      const int toff = traj_offset + t0;
      // with the overlap: on the side stream, once the trajectories of block b-2 are done with this half, and `s` waits for the draws
      const hipStream_t ms = ov ? ov->side : s;
      if (ov) { if (bidx >= 2) (void)hipStreamWaitEvent(ov->side, ov->freed[bidx & 1], 0); }
      else profile_begin(s);
      if (draw == Draw::split) {
        const size_t slds = momentum_split_lds_elems(D) * sizeof(T);
        const int64_t sg = (ntask + 3) / 4;
        const int64_t sres = (int64_t)fused_cu_count() * (slds <= 52 * 1024 ? 3 : (slds <= 78 * 1024 ? 2 : 1));   // resident workgroups: L_P is staged once each
        rmhmc_momentum_split_kernel<T><<<(int)(sg < sres ? sg : sres), 256, slds, ms>>>(LP, (T)jitter, C, D, nt, toff, seed, chain_offset, p_blk);
      } else if (draw == Draw::wave) {
        if constexpr (sizeof(T) == 4) {
          const int wgrid = (int)(ntask < 256 * 16 ? ntask : 256 * 16);
          auto wave = [&](auto NB) {
            rmhmc_momentum_wave_kernel<decltype(NB)::value><<<wgrid, 64, 0, ms>>>(P, (float)jitter, C, D, nt, toff, seed, chain_offset, p_blk);
          };
          const int nb = (D + 7) / 8;
          if (nb <= 4) wave(std::integral_constant<int, 4>{});
          else if (nb <= 7) wave(std::integral_constant<int, 7>{});
          else if (nb <= 10) wave(std::integral_constant<int, 10>{});
          else wave(std::integral_constant<int, 13>{});
        }
      } else {
        const int mgrid = (int)(ntask < 256 * 12 ? ntask : 256 * 12);
        rmhmc_momentum_kernel<T><<<mgrid, FNT, momentum_lds_elems(D, ld) * sizeof(T), ms>>>(P, has_jitter, (T)jitter, C, D, ld, nt, toff, seed, chain_offset, p_blk);
      }
      if (ov) {
        (void)hipEventRecord(ov->ready[bidx & 1], ov->side);
        (void)hipStreamWaitEvent(s, ov->ready[bidx & 1], 0);
      } else profile_end(s);
    }
    FusedArgs<T> a{cur, theta_init, P, Sinv, mu, (T)log_norm, (T)logdetP, has_jitter, (T)jitter, K, series, C, D, L, (T)eps,
                   (T)cosf(ang), (T)sinf(ang), nt, traj_offset + t0, burn, seed, chain_offset, samples, reject_count,
                   H_old ? H_old + (int64_t)t0 * C : nullptr, H_new ? H_new + (int64_t)t0 * C : nullptr,
                   accept ? accept + (int64_t)t0 * C : nullptr, block > 0 ? p_blk : nullptr};
    // two chains per workgroup (NC = 2; needs pre-drawn momenta and the log-det series): measured 5 % SLOWER than one
    // chain per workgroup at 1024 and 4096 chains (the pass is LDS-bandwidth bound: every wave streams every vector), so it
    // is only taken on request (tuning value 3: parity tests keep the variant alive)
    const bool pair = g_rmhmc_fused == 3 && lean;
    const bool need_w = !lean;                                         // a Cholesky inside the kernel: work matrix in LDS
    auto trajectories = [&]() -> int {
      if constexpr (sizeof(T) == 4) {
        // one or two chains per workgroup, their state sets as columns of the 16-block matrix instruction (rmhmc_uv.hip): up to
        // 2 x (compute units) chains (tuning key "rmhmc_uv": 0 off, 2 at any chain count)
        const bool uv = g_rmhmc_uv && g_rmhmc_mfma4 != 2 && g_rmhmc_batch != 2 && !pair && lean && D <= QK &&
                        (C <= (g_rmhmc_uv_co ? 7 : 2) * (int64_t)fused_cu_count() || g_rmhmc_uv == 2);
        if (uv) {
          profile_begin(s);
          const int rc_uv = rmhmc_uv_launch(a, fused_cu_count(), s);
          profile_end(s);
          return rc_uv;
        }
        // four chains per workgroup on the 16-block matrix instruction: C / 4 two-wave workgroups (tuning key "rmhmc_mfma4")
        const bool quad4 = g_rmhmc_mfma4 && !pair && lean && D <= QK && ((C >= g_rmhmc_mfma4_lo && C < g_rmhmc_mfma4_hi) || g_rmhmc_mfma4 == 2);
        if (quad4) {
          const int64_t ngroup = (C + QNC - 1) / QNC;
          const int qgrid = (int)(ngroup < 8192 ? ngroup : 8192);
          profile_begin(s);
          note_route("rmhmc_mfma4_kernel<%s>", g_rmhmc_pair ? "true" : "false");
          with_track([&](auto TRACK) -> int {
            rmhmc_mfma4_kernel<decltype(TRACK)::value><<<qgrid, QNT, Mfma4Tile::LDS_FLOATS * sizeof(float), s>>>(a);
            return HTA_OK;
          });
          profile_end(s);
          return HTA_OK;
        }
        // sixteen chains per workgroup on the 16 x 16 tiles (tuning key "rmhmc_batch"); one workgroup per CU
        const bool batch = g_rmhmc_batch && !pair && lean && D <= 16 * BWV && (C >= 2048 || g_rmhmc_batch == 2);
        if (batch) {
          const int64_t ngroup = (C + BNC - 1) / BNC;
          const int bgrid = (int)(ngroup < 4096 ? ngroup : 4096);
          return with_track([&](auto TRACK) -> int {
            constexpr bool TR = decltype(TRACK)::value;
            static DevOnce done_b;                               // the four instances opt in together
            if (const int rc = allow_big_lds(done_b, kEntry, &rmhmc_batch_kernel<25, true>, &rmhmc_batch_kernel<28, true>,
                                             &rmhmc_batch_kernel<25, false>, &rmhmc_batch_kernel<28, false>))
              return rc;
            profile_begin(s);
            note_route("rmhmc_batch_kernel<%d,%s>", D <= 100 ? 25 : 28, TR ? "true" : "false");
            if (D <= 100) rmhmc_batch_kernel<25, TR><<<bgrid, BNT, BatchTile<25>::LDS_FLOATS * sizeof(float), s>>>(a);
            else rmhmc_batch_kernel<28, TR><<<bgrid, BNT, BatchTile<28>::LDS_FLOATS * sizeof(float), s>>>(a);
            profile_end(s);
            return HTA_OK;
          });
        }
        // one chain per workgroup, at most one workgroup per CU: the spill-free instances (tuning key "rmhmc_wide")
        if (!pair && g_rmhmc_wide && (KH == 56 || KH == 64) && C <= fused_cu_count()) {
          return with_track([&](auto TRACK) -> int {
            constexpr bool TR = decltype(TRACK)::value;
            static DevOnce done_w[2];                            // per instance
            const auto wide = KH == 56 ? &rmhmc_fused_kernel_wide<56, TR> : &rmhmc_fused_kernel_wide<64, TR>;
            if (const int rc = allow_big_lds(done_w[KH == 64], kEntry, wide)) return rc;
            profile_begin(s);
            note_route("rmhmc_fused_kernel_wide<%d,%s>", KH, TR ? "true" : "false");
            wide<<<grid, FNT, fused_lds_bytes<T>(D, nullptr, 1, need_w), s>>>(a, ld, need_w ? 1 : 0);
            profile_end(s);
            return HTA_OK;
          });
        }
      }
      // one chain per workgroup or, on request, two.  The once-flags are statics of the generic callable: one per instance.
      return with_kh(KH, [&](auto KHC) -> int {
        return with_track([&](auto TRACK) -> int {
          constexpr auto kern = &rmhmc_fused_kernel<T, decltype(KHC)::value, 1, decltype(TRACK)::value>;
          constexpr auto kern2 = &rmhmc_fused_kernel<T, decltype(KHC)::value, 2>;
          static DevOnce done, done2;
          if (const int rc = pair ? allow_big_lds(done2, kEntry, kern2) : allow_big_lds(done, kEntry, kern)) return rc;
          profile_begin(s);
          if (pair) {
            const int64_t npair = (C + 1) / 2;
            note_route("rmhmc_fused_kernel<%s,%d,2>", tname, KH);
            kern2<<<(int)(npair < 8192 ? npair : 8192), FNT, fused_lds_bytes<T>(D, nullptr, 2, false), s>>>(a, ld, 0);
          } else {
            note_route("rmhmc_fused_kernel<%s,%d,1,%s>", tname, KH, decltype(TRACK)::value ? "true" : "false");
            kern<<<grid, FNT, fused_lds_bytes<T>(D, nullptr, 1, need_w), s>>>(a, ld, need_w ? 1 : 0);
          }
          profile_end(s);
          return HTA_OK;
        });
      });
    };
    if (const int rc = trajectories()) return rc;
    if (ov) (void)hipEventRecord(ov->freed[bidx & 1], s);
  }
  HTA_CHECK_LAUNCH("hta_rmhmc_gaussian_sample (fused)");
  return HTA_OK;
}

template <typename T> int inverse_from_eigen(const T* V0, const T* lam0, T* S, int D, hipStream_t s) {
  inverse_from_eigen_kernel<T><<<1, 1024, 0, s>>>(V0, lam0, S, D);
  HTA_CHECK_LAUNCH("hta_rmhmc_gaussian_sample (inverse)");
  return HTA_OK;
}

#define HTA_INST(T)                                                                                                   \
  template int fused_plan<T>(const T*, int, int, double, int, double, double*, int*);                                 \
  template int inverse_from_eigen<T>(const T*, const T*, T*, int, hipStream_t);                                       \
  template int rmhmc_fused_sample<T>(T*, const T*, const T*, const T*, const T*, double, double, int, double, int,   \
                                     int, int64_t, int, int, double, double, int, int, int, uint64_t, uint64_t, T*,   \
                                     int32_t*, T*, T*, uint8_t*, T*, int64_t, const T*, hipStream_t);
HTA_INST(float)
HTA_INST(double)

}  // namespace hta
