// Fused (split-)HMC for SMALL fully connected Bayesian networks of any depth: 1 .. 4 Linear layers (none to three hidden ones),
// one activation kind between them, Gaussian / Bernoulli-with-logits / softmax-cross-entropy likelihood.
// Same contract as mlp_hmc.hip (hamiltorch/samplers.py:965-1026 trajectory loop, S:1141-1199 closures, S:499-596 split
// integrators, S:281-302 leapfrog); what it adds are the shapes the reference's notebooks actually sample: the two-hidden-layer
// regression net of the split-HMC notebook (1-10-10-1), the softmax regression of the BNN notebook (Linear(4, 3),
// `multi_class_linear_output`, the default `model_loss` of sample_model) and small classifiers with several outputs.
//
// Work layout.  These nets have tens to a few hundred parameters and layers 1 .. 32 wide: nothing for a matrix core to hold on
// to, but a data set of hundreds of points.  ONE WAVE PER CHAIN, lanes = points: a lane carries its point through the layers
// (activations and deltas of the point in this lane's column of two small LDS matrices, [unit][lane]: conflict-free), the
// parameters of the chain are a broadcast operand (one LDS copy per wave, every lane reads the same address).  A weight's
// gradient sum_p delta[p][o] a[p][i] is a sum of outer products over the points: in fp32 it runs on the matrix cores
// (v_mfma_f32_4x4x1_16b_f32: the weight matrices of all layers, bias columns included, cut into 4 x 4 blocks, 16 blocks per
// instruction - one or a few instructions per point, blocks accumulated in registers over a whole pass; pass()), in fp64 it
// is a reduction over the lanes per weight.  Leapfrog state (q, p, gradient, masses) lives in registers, parameter
// 64 k + lane in register k of lane `lane`.  One wave per workgroup: barriers cost nothing, 1024 chains put a wave on every SIMD.
// How it got here (tools/history/netn_time.py, profiles/r02z_netn_speed.txt; Net([1,10,10,1]), 400 points, 1024 chains):
// 3.6e6 chain-steps/s with one point per lane and a DPP reduction per weight -> 5.4e6 (interleaved reductions, plain ds_add) ->
// 8.6e6 (several points per lane, blocks of four units) -> 1.46e7 (gradient on the matrix cores); the callback path: 6.8e5.
// Tried and dropped: the forward products and the delta propagation as matrix instructions as well ((4 points) x (4 units)
// blocks, the lane's own activation as the A operand, the result written back transposed inside the quad): 1.16e7 - its
// per-input loop with run-time layer shapes issues more than the blocked FMA loops it replaces.
// Layer shapes are run-time values (uniform loops); limits: D <= 512 parameters, widths <= 64, N <= what L2 holds (X is read
// from global memory, coalesced over the lanes).
//
// This file: the tuning key, the argument checks, the choice of waves per chain and points per lane, the launcher and the C
// entry points.  The kernel: netn_hmc_dev.hpp.
#include "netn_hmc_dev.hpp"

namespace hta {

int g_netn_waves = 1;      // tuning key "netn_waves": waves per chain (2 / 4 where they fit; measured slower at 1024 chains)

// what netn_hmc() works out for a launch, and the launch of one instance (its once-flag is a static of the instance)
struct NetnLaunch { int D, SW, WM, grid; size_t lds; };
template <typename T, int PB, int WV> static int launch_netn(const NetArgs<T>& a, const NetnLaunch& g, hipStream_t s) {
  static DevOnce done;
  if (const int rc = allow_big_lds(done, "hta_netn_hmc", &netn_hmc_kernel<T, PB, WV>)) return rc;
  profile_begin(s);
  note_route("netn_hmc_kernel<%s,%d,%d>", sizeof(T) == 4 ? "float" : "double", PB, WV);
  netn_hmc_kernel<T, PB, WV><<<g.grid, 64 * WV, g.lds, s>>>(a, g.D, g.SW, g.WM);
  profile_end(s);
  HTA_CHECK_LAUNCH("hta_netn_hmc");
  return HTA_OK;
}

template <typename T> int netn_hmc(const NetArgs<T>& a, hipStream_t s) {
  HTA_REQUIRE(a.theta && a.X && a.Y && a.C > 0, "hta_netn_hmc: NULL pointer / empty batch");
  if constexpr (sizeof(T) == 4) {          // two wide hidden layers, one output, Gaussian likelihood: the matrix-core kernel (mlp3_mfma.hip)
    if (a.n_layers == 3 && mlp3_eligible(a)) return mlp3_mfma(a, s);
  }
  HTA_REQUIRE(a.n_layers >= 1 && a.n_layers <= NETN_MAX_LAYERS, "hta_netn_hmc: %d Linear layers not in [1, %d]", a.n_layers, NETN_MAX_LAYERS);
  int D = 0, SW = a.dims[0], WM = 1;
  for (int l = 0; l <= a.n_layers; ++l)
    HTA_REQUIRE(a.dims[l] >= 1 && a.dims[l] <= NETN_MAX_WIDTH, "hta_netn_hmc: layer width %d not in [1, %d]", a.dims[l], NETN_MAX_WIDTH);
  for (int l = 0; l < a.n_layers; ++l) {
    D += a.dims[l] * a.dims[l + 1] + a.dims[l + 1];
    SW += a.dims[l + 1];
    if (a.dims[l + 1] > WM) WM = a.dims[l + 1];
    if (a.dims[l] > WM) WM = a.dims[l];
  }
  HTA_REQUIRE(D <= 64 * NETN_KMAX, "hta_netn_hmc: %d parameters exceed the native limit of %d", D, 64 * NETN_KMAX);
  HTA_REQUIRE(a.act >= 0 && a.act <= 2, "hta_netn_hmc: unknown activation %d", a.act);
  HTA_REQUIRE(a.loss == HTA_LOSS_REGRESSION || a.loss == HTA_LOSS_BINARY_LOGITS || a.loss == HTA_LOSS_SOFTMAX_CE,
              "hta_netn_hmc: unknown loss kind %d", a.loss);
  if (const int rc = check_split_args(a, "hta_netn_hmc", "hta_netn_logp_grad")) return rc;
  // Waves per chain (WV) and points per lane (PB), from the size of a GRADIENT pass (Nb points; the two full-data log p passes
  // of a trajectory are the minority).  A sweep of a wave covers 64 PB points.  Both: the largest of 4, 2, 1 that a pass keeps
  // more than half busy - while the LDS footprint still lets every chain of the launch be resident (a second round of
  // workgroups costs more than either buys: at 1024 chains four workgroups share a CU).
  const int Dp = (D + 63) & ~63;
  auto lds_for = [&](int pb, int wv) {
    return ((size_t)2 * Dp + 4 + (size_t)wv * 2 * (SW + 2) * (64 * pb + 1)) * sizeof(T) + 64 * sizeof(int);
  };
  if (sizeof(T) == 4) {                                     // the matrix-core gradient holds at most 16 NETN_NSET blocks of 4 x 4
    int nb = 0;
    for (int l = 0; l < a.n_layers; ++l) nb += ((a.dims[l + 1] + 3) / 4) * ((a.dims[l] + 4) / 4);
    HTA_REQUIRE(nb <= 16 * NETN_NSET, "hta_netn_hmc: %d blocks of 4 x 4 weights exceed the native limit of %d", nb, 16 * NETN_NSET);
  }
  int cus = 256;
  {
    int dev = 0; hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
  }
  auto resident = [&](int pb, int wv) {
    const size_t per_cu = (size_t)(150 * 1024) / lds_for(pb, wv);
    const size_t by_waves = (size_t)32 / wv;                // 8 waves per SIMD at most
    return (int64_t)cus * (int64_t)(per_cu < by_waves ? per_cu : by_waves);
  };
  // Measured (profiles/r02z_netn_speed.txt): more waves per chain LOSE at 1024 chains - 1.46e7 -> 1.11e7 chain-steps/s on
  // Net([1,10,10,1]) with two waves and one point per lane instead of one wave and two points, 7.9e7 -> 4.3e7 on the softmax
  // regression with four: the real barriers and the LDS exchange cost more than the second wave's latency hiding buys (the
  // RMHMC kernels found the same).  So one wave per chain unless the tuning key "netn_waves" asks for more.
  int WV = g_netn_waves >= 4 ? 4 : (g_netn_waves >= 2 ? 2 : 1), PB = 4;
  while (WV > 1 && (a.Nb <= 32 * WV || resident(1, WV) < a.C)) WV >>= 1;
  while (PB > 1 && (a.Nb <= 32 * PB * WV || resident(PB, WV) < a.C)) PB >>= 1;
  const size_t lds = lds_for(PB, WV);
  HTA_REQUIRE(lds <= 150 * 1024, "hta_netn_hmc: the layer widths need %zu bytes of LDS", lds);
  const int grid = (int)(a.C < 65536 ? a.C : 65536);
  const NetnLaunch g{D, SW, WM, grid, lds};
  switch (10 * PB + WV) {
    case 11: return launch_netn<T, 1, 1>(a, g, s);
    case 12: return launch_netn<T, 1, 2>(a, g, s);
    case 14: return launch_netn<T, 1, 4>(a, g, s);
    case 21: return launch_netn<T, 2, 1>(a, g, s);
    case 22: return launch_netn<T, 2, 2>(a, g, s);
    case 24: return launch_netn<T, 2, 4>(a, g, s);
    case 41: return launch_netn<T, 4, 1>(a, g, s);
    case 42: return launch_netn<T, 4, 2>(a, g, s);
    case 44: return launch_netn<T, 4, 4>(a, g, s);
  }
  set_error("hta_netn_hmc: internal error: no instance for PB=%d, WV=%d", PB, WV);    // unreachable: both are 1, 2 or 4
  return HTA_ERR_INVALID;
}

template <typename T>
static int netn_fill(NetArgs<T>& a, int n_layers, const int* dims, const T* taus) {
  if (!dims || !taus) { set_error("hta_netn: dims / taus is NULL (host pointers)"); return HTA_ERR_INVALID; }
  if (n_layers < 1 || n_layers > NETN_MAX_LAYERS) { set_error("hta_netn: %d Linear layers not in [1, %d]", n_layers, NETN_MAX_LAYERS); return HTA_ERR_INVALID; }
  a.n_layers = n_layers;
  for (int l = 0; l <= NETN_MAX_LAYERS; ++l) a.dims[l] = l <= n_layers ? dims[l] : 0;
  for (int l = 0; l < 2 * NETN_MAX_LAYERS; ++l) a.tau[l] = l < 2 * n_layers ? taus[l] : (T)1;
  return HTA_OK;
}

}  // namespace hta

extern "C" {
#define HTA_DEFINE_NETN(SUF, T)                                                                                          \
  int hta_netn_hmc_sample_##SUF(T* theta, const T* theta_init, int64_t C, int n_layers, const int* dims, int act,        \
                                int loss_kind, const T* X, const T* Y, int N, int M, int Nb, const T* taus, T tau_out,   \
                                T prior_scale, int mass_kind, const T* inv_mass, const T* mass_factor, int integrator,   \
                                int L, T eps, int n_traj, int traj_offset, int burn, uint64_t seed, uint64_t chain_offset, \
                                T* samples, int32_t* reject_count, T* H_old, T* H_new, uint8_t* accept, void* workspace, \
                                int64_t workspace_bytes, void* stream) {                                                 \
    hta::NetArgs<T> a{};                                                                                                 \
    if (int rc = hta::netn_fill<T>(a, n_layers, dims, taus)) return rc;                                                  \
    a.theta = theta; a.theta_init = theta_init; a.C = C; a.act = act; a.loss = loss_kind; a.X = X; a.Y = Y; a.N = N;      \
    a.M = M; a.Nb = Nb; a.tau_out = tau_out; a.prior_scale = prior_scale; a.mass_kind = mass_kind; a.inv_mass = inv_mass; \
    a.mass_factor = mass_factor; a.L = L; a.eps = eps; a.n_traj = n_traj; a.traj_offset = traj_offset; a.burn = burn;    \
    a.seed = seed; a.chain_offset = chain_offset; a.samples = samples; a.reject_count = reject_count; a.H_old = H_old;   \
    a.H_new = H_new; a.accept = accept; a.integ = integrator; a.workspace = workspace; a.workspace_bytes = workspace_bytes; \
    if (n_traj <= 0) return HTA_OK;                                                                                      \
    return hta::netn_hmc<T>(a, (hipStream_t)stream);                                                                     \
  }                                                                                                                      \
  int hta_netn_logp_grad_##SUF(const T* theta, int64_t C, int n_layers, const int* dims, int act, int loss_kind, const T* X, \
                               const T* Y, int N, int M, int Nb, int split, const T* taus, T tau_out, T prior_scale,     \
                               T* grad_out, T* logp_out, void* workspace, int64_t workspace_bytes, void* stream) {       \
    hta::NetArgs<T> a{};                                                                                                 \
    if (int rc = hta::netn_fill<T>(a, n_layers, dims, taus)) return rc;                                                  \
    a.theta = const_cast<T*>(theta); a.C = C; a.act = act; a.loss = loss_kind; a.X = X; a.Y = Y; a.N = N; a.M = M;        \
    a.Nb = Nb; a.tau_out = tau_out; a.prior_scale = prior_scale; a.mass_kind = HTA_MASS_NONE; a.grad_out = grad_out;     \
    a.logp_out = logp_out; a.eval_split = split; a.integ = HTA_SPLIT_SYMMETRIC; a.workspace = workspace;                 \
    a.workspace_bytes = workspace_bytes;                                                                                 \
    return hta::netn_hmc<T>(a, (hipStream_t)stream);                                                                     \
  }
HTA_DEFINE_NETN(f32, float)
HTA_DEFINE_NETN(f64, double)
#undef HTA_DEFINE_NETN

int64_t hta_netn_hmc_workspace_bytes(int64_t C, int n_layers, const int* dims, int elem_size) {
  return elem_size == 4 ? hta::mlp3_workspace_bytes(C, n_layers, dims) : 0;      /* the one-wave-per-chain kernels need none */
}
}
