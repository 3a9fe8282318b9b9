// Fused (split-)HMC for a one-hidden-layer Bayesian MLP with a Gaussian (regression) likelihood, any dtype and shape
// (n_in <= 32, H <= 1024): the fp64 / wide-layer route, and the fp32 parity partner (tuning key "mlp_valu") of
// mlp_mfma.hip, which runs BASELINE config 4.  One workgroup per chain; the whole trajectory loop of sample()
// (hamiltorch/samplers.py:965-1026) runs on-chip with
//   log p_m(theta) = -1/2 tau_out sum_{i in split m} (f(x_i) - y_i)^2
//                    + (1/prior_scale) sum_layers Normal(0, tau_l^-1/2).log_prob(w).sum()
// (define_model_log_prob, S:1141-1199; one closure per DataLoader batch, S:1251-1255) and either
//   * the symmetric split integrator (S:499-540): 2M gradient half-kicks + 2(M-1) drifts per step, or
//   * plain leapfrog over the full data (S:281-302) when M == 1 (sample_model).
//
// Work layout.  theta = [W1[H,in] | b1[H] | W2[1,H] | b2[1]] (U:121-122 order).  Wave (g, s): lane l is
// hidden unit j = 64 g + l, the wave is point slice s of PS; the unit's weights, momentum and gradient
// live in its registers (replicated over the PS slice waves, which stay bit-identical).  Because a wave
// works on ONE data point at a time, x_i is wave-uniform: it comes through the scalar cache
// (s_load_dwordx8) straight into SGPR operands of v_pk_fma_f32 - no LDS or vector-memory traffic for
// the data set at all.  A gradient of one data chunk is two passes over the chunk's points:
//   1. h_ij = act(b1_j + W1_j . x_i) -> LDS [i][j];  4 lanes per row form f(x_i) = b2 + sum_j W2_j h_ij
//      (float4 reads), the residual and delta_i = -tau_out (f(x_i) - y_i)  (LDS vector);
//   2. every wave re-reads h_ij of its points and accumulates dW2_j, db1_j, dW1_j. in registers
//      (packed FMAs, x_i from SGPRs); one LDS exchange sums the PS slice partials per gradient.
// HBM traffic per trajectory: one [D] sample row per chain.
//
// This file: the tuning key, the LDS sizing, the launcher and the C entry points.  The kernel: mlp_hmc_dev.hpp.
// One build switch: -DHTA_MLP_SINGLE (here and in mlp_mfma.hip) builds one instantiation, for the CPU resource test.
#include "mlp_hmc_dev.hpp"

namespace hta {

int g_mlp_valu = 0;      // tuning key "mlp_valu": 1 = keep the Bayesian-MLP sampler on this VALU kernel (parity tests of both)

template <typename T, int INMAX, int NT, int ACT, bool EXACT> int launch_mlp_act(const MlpArgs<T>& a, hipStream_t s) {
  // waves: UG groups of 64 hidden units x PS point slices
  const int UG = (a.H + 63) / 64, PS = (NT / 64) / UG;
  const int Hp = (a.H + 15) / 16 * 16;                 // row-sum lanes read float4 x 4 lanes
  int ldc = UG * 64;                                   // every lane of a unit group owns a column: unconditional stores
  while (ldc % 32 != 16) ldc += 4;                     // 4 consecutive rows land on distinct bank quarters
  typedef MlpChain<T, INMAX, NT, ACT, EXACT> Ch;
  const size_t recs = (size_t)NT * Ch::GS;             // slice-exchange / momentum-draw records, aliasing the chunk matrix
  const size_t fixed = ((size_t)Hp + a.N + 2 * (NT / 64) + 8 + 64) * sizeof(T);        // ... + 64 ints: subset order
  const size_t cap = 150 * 1024;
  HTA_REQUIRE(fixed + (recs + 4) * sizeof(T) <= cap && fixed + (size_t)4 * (ldc + 1) * sizeof(T) <= cap,
              "hta_mlp_hmc: data set (N=%d) / hidden layer (H=%d) do not fit the LDS staging", a.N, a.H);
  int nbch = (int)((cap - fixed) / ((ldc + 1) * sizeof(T)));
  if (nbch > a.Nb) nbch = a.Nb;
  if (nbch > 256) nbch = 256;
  HTA_REQUIRE(nbch >= 1, "hta_mlp_hmc: no LDS left for the chunk matrix");
  size_t cmsz = (size_t)nbch * ldc;
  if (cmsz < recs) cmsz = recs;
  const size_t lds = fixed + (cmsz + nbch) * sizeof(T);
  static DevOnce done;
  if (const int rc = allow_big_lds(done, "hta_mlp_hmc", &mlp1_hmc_kernel<T, INMAX, NT, ACT, EXACT>)) return rc;
  const int grid = (int)(a.C < 4096 ? a.C : 4096);
  profile_begin(s);
  note_route("mlp1_hmc_kernel<%s,%d,%d,%d,%s>", sizeof(T) == 4 ? "float" : "double", INMAX, NT, ACT, EXACT ? "true" : "false");
  mlp1_hmc_kernel<T, INMAX, NT, ACT, EXACT><<<grid, NT, lds, s>>>(a, nbch, ldc, (int)cmsz, Hp, PS, UG);
  profile_end(s);
  HTA_CHECK_LAUNCH("hta_mlp_hmc");
  return HTA_OK;
}

template <typename T, int INMAX, int NT, bool EXACT> int launch_mlp_x(const MlpArgs<T>& a, hipStream_t s) {
  if (a.act == 0) return launch_mlp_act<T, INMAX, NT, 0, EXACT>(a, s);
  if (a.act == 1) return launch_mlp_act<T, INMAX, NT, 1, EXACT>(a, s);
  return launch_mlp_act<T, INMAX, NT, 2, EXACT>(a, s);
}

template <typename T, int INMAX, int NT> int launch_mlp(const MlpArgs<T>& a, hipStream_t s) {
  if (a.n_in == INMAX) return launch_mlp_x<T, INMAX, NT, true>(a, s);
  return launch_mlp_x<T, INMAX, NT, false>(a, s);
}

template <typename T, int INMAX> int dispatch_ps(const MlpArgs<T>& a, hipStream_t s) {
  if (a.H <= 512) return launch_mlp<T, INMAX, 512>(a, s);
  return launch_mlp<T, INMAX, 1024>(a, s);
}

template <typename T> int mlp_hmc(const MlpArgs<T>& a, hipStream_t s) {
  HTA_REQUIRE(a.theta && a.X && a.Y && a.C > 0, "hta_mlp_hmc: NULL pointer / empty batch");
  HTA_REQUIRE(a.n_in >= 1 && a.n_in <= 32, "hta_mlp_hmc: input width %d not in [1, 32]", a.n_in);
  HTA_REQUIRE(a.H >= 1 && a.H <= 1024, "hta_mlp_hmc: hidden width %d not in [1, 1024]", a.H);
  HTA_REQUIRE(a.act >= 0 && a.act <= 2, "hta_mlp_hmc: unknown activation %d", a.act);
  HTA_REQUIRE(a.loss == HTA_LOSS_REGRESSION || a.loss == HTA_LOSS_BINARY_LOGITS, "hta_mlp_hmc: unknown loss kind %d", a.loss);
  if (const int rc = check_split_args(a, "hta_mlp_hmc", "hta_mlp_logp_grad")) return rc;
  if constexpr (sizeof(T) == 4) {
    if (!g_mlp_valu && mlp_mfma_eligible(a)) return mlp_mfma(a, s);
  }
#ifdef HTA_MLP_SINGLE       // one instantiation (the BASELINE config-4 shape), seconds to compile: the CPU resource test
  return launch_mlp_act<T, 8, 512, 0, true>(a, s);
#else
  if (a.n_in <= 4) return dispatch_ps<T, 4>(a, s);
  if (a.n_in <= 8) return dispatch_ps<T, 8>(a, s);
  if (a.n_in <= 16) return dispatch_ps<T, 16>(a, s);
  return dispatch_ps<T, 32>(a, s);
#endif
}

}  // namespace hta

extern "C" {
#define HTA_DEFINE_MLP(SUF, T)                                                                                    \
  int hta_mlp_hmc_sample_##SUF(T* theta, const T* theta_init, int64_t C, int n_in, int H, int act, int loss_kind, const T* X, \
                               const T* Y, int N, int M, int Nb, const T* tau4, T tau_out, T prior_scale,           \
                               int mass_kind, const T* inv_mass, const T* mass_factor, int integrator, int L,      \
                               T eps, int n_traj, int traj_offset, int burn, uint64_t seed, uint64_t chain_offset, \
                               T* samples,                                                                          \
                               int32_t* reject_count, T* H_old, T* H_new, uint8_t* accept, void* stream) {          \
    if (!tau4) { hta::set_error("hta_mlp_hmc_sample: tau4 is NULL (host pointer to 4 precisions)"); return HTA_ERR_INVALID; } \
    hta::MlpArgs<T> a{theta, theta_init, C, n_in, H, act, X, Y, N, M, Nb, {tau4[0], tau4[1], tau4[2], tau4[3]},     \
                      tau_out, prior_scale, mass_kind, inv_mass, mass_factor, L, eps, n_traj, traj_offset, burn,    \
                      seed, chain_offset, samples, reject_count, H_old, H_new, accept, nullptr, nullptr, 0,         \
                      integrator, loss_kind};                                                                       \
    if (n_traj <= 0) return HTA_OK;                                                                                 \
    return hta::mlp_hmc<T>(a, (hipStream_t)stream);                                                                 \
  }                                                                                                                 \
  int hta_mlp_logp_grad_##SUF(const T* theta, int64_t C, int n_in, int H, int act, int loss_kind, const T* X, const T* Y, int N, \
                              int M, int Nb, int split, const T* tau4, T tau_out, T prior_scale, T* grad_out,       \
                              T* logp_out, void* stream) {                                                          \
    if (!tau4) { hta::set_error("hta_mlp_logp_grad: tau4 is NULL"); return HTA_ERR_INVALID; }                       \
    hta::MlpArgs<T> a{const_cast<T*>(theta), nullptr, C, n_in, H, act, X, Y, N, M, Nb,                              \
                      {tau4[0], tau4[1], tau4[2], tau4[3]}, tau_out, prior_scale, HTA_MASS_NONE, nullptr, nullptr,  \
                      0, (T)0, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, grad_out, logp_out,      \
                      split, HTA_SPLIT_SYMMETRIC, loss_kind};                                                       \
    return hta::mlp_hmc<T>(a, (hipStream_t)stream);                                                                 \
  }
HTA_DEFINE_MLP(f32, float)
HTA_DEFINE_MLP(f64, double)
}
