// Fused (split-)HMC for a Bayesian MLP with TWO wide hidden layers, fp32 on the gfx950 matrix cores:
//     Linear(n_in, H1) - act - Linear(H1, H2) - act - Linear(H2, 1),  Gaussian likelihood,  n_in <= 4,  H1, H2 <= 104.
// This is the one model the reference publishes a GPU number for - notebooks/hamiltorch_split_HMC_BNN_example.ipynb cell 9:
// Linear(1,100)-ReLU-Linear(100,100)-ReLU-Linear(100,1), D = 10401, 400 points in M = 4 splits, L = 30, eps = 5e-4
// (13.47 samples/s full HMC, 1.83 samples/s symmetric split HMC on an RTX 2080 Max-Q, one chain).
// Same contract as mlp_mfma.hip / netn_hmc.hip: hamiltorch/samplers.py:965-1026 (trajectory loop), S:1141-1199 (closures of
// define_model_log_prob / define_split_model_log_prob), S:499-596 (split integrators), S:281-302 (leapfrog).
//
// Cost of a gradient: three (points x H) x (H x H) products - Z2 = A1 W2^T, dW2 = delta2^T A1, delta1 = delta2 W2 -
// 6 N_b H1 H2 flop, 100 x the element-wise work of the thin first and last layers: a GEMM problem, v_mfma_f32_16x16x4_f32
// (exact fp32).  ONE WORKGROUP OF 7 WAVES PER CHAIN; wave w owns the 16 second-layer units 16 w .. 16 w + 15 and the 16
// first-layer units of the same indices; lane l = (g = l >> 4, c = l & 15).
//
// State in registers.  theta, p and the gradient of a chain live in VGPRs for the whole launch.  The 100 x 100 matrix W2 is
// held as 7 x 4 registers per lane in the OPERAND layout of the forward product: lane (g, c) of wave w keeps row
// u = 16 w + c, register [s][t] <-> column j = 16 s + 4 g + t (s < 6; the last block is j = 96 + 4 t + g).  A matrix
// instruction sums over its 4 K slots in any order, so a block of 16 contraction indices is consumed by 4 instructions whose
// K slot g at step t is index 16 s + 4 g + t: BOTH operands of a step are then one 16-byte LDS read (ds_read_b128, rows
// padded to 104 / 120 floats: conflict free) per FOUR instructions, instead of one 4-byte read per instruction.
//   forward  Z2[p, u]  = b2_u + sum_j A1[p, j] W2[u, j]    A = A1[p][.] from LDS, B = the theta registers themselves
//   dW2^T[j, u]        = sum_p A1[p, j] delta2[p, u]        A = A1T[j][.] from LDS, B = delta2 AS IT LIES in the forward
//                        accumulator (C layout: lane (g, c) register r = point 4 g + r, unit c = K slot g, step r); the
//                        result's C layout (row j = 16 s + 4 g + r, column u = 16 w + c) IS the theta register layout, so kick
//                        and drift of W2 are element-wise register operations
//   delta1[p, j]       = sum_u delta2[p, u] W2[u, j]        A = delta2[p][.] from LDS, B = W2 re-read column-wise from a
//                        staging copy (7 x 4 more registers, refreshed once per gradient)
// f(x_p) = b3 + sum_u w3_u a2[p, u]: reduce-scatter over the 16 unit lanes (DPP), over the waves through LDS.  The thin layers
// (W1, b1, b2, w3, b3: 401 of 10401 parameters) are per-unit registers with copies in the 4 lane groups.
// LDS (151 KB): A1 [112][104] | D2 [112][104] (delta2; doubles as the W2 staging copy) | A1T [112][120] | X, Y of the chunk | partials.
//
// This file: the tuning key, eligibility, the LDS and workspace sizing, the launcher.  The kernel: mlp3_mfma_dev.hpp.
#include "mlp3_mfma_dev.hpp"

namespace hta {

int g_mlp3_route = 1;      // tuning key "mlp3_route": 0 = such models stay on the callback path, 2 = also the shapes the small-net kernel holds

static size_t mlp3_lds_floats() {          // without the data set
  return (size_t)2 * M3_CP * M3_LDJ + (size_t)M3_CP * M3_LDP + M3_NIN * M3_CP + M3_CP + M3_NW * M3_CP + M3_CP + 16 + 64;
}
// padded length of the LDS copy of the data set, or 0 when it does not fit (or the 16-byte reads of a chunk would be
// misaligned: every chunk starts at m Nb + 112 i): then every pass stages its chunk from global memory
static int mlp3_data_np(const NetArgs<float>& a) {
  const int NP = (a.N + 3) / 4 * 4 + M3_CP;
  if (a.Nb % 4 != 0) return 0;
  return (mlp3_lds_floats() + (size_t)(a.dims[0] + 1) * NP) * sizeof(float) <= 160 * 1024 ? NP : 0;
}

// the layer shapes of this route: n_in-H1-H2-1 within the kernel's limits and beyond the small-net kernel's
static bool mlp3_shape(int n_layers, const int* dims) {
  if (n_layers != 3 || dims[3] != 1) return false;
  if (dims[0] < 1 || dims[0] > M3_NIN || dims[1] < 1 || dims[1] > M3_HMAX || dims[2] < 1 || dims[2] > M3_HMAX) return false;
  // the small-net kernel (one wave per chain) keeps what it can hold: widths <= 64 and <= 512 parameters
  const int D = dims[0] * dims[1] + dims[1] + dims[1] * dims[2] + 2 * dims[2] + 1;
  return dims[1] > NETN_MAX_WIDTH || dims[2] > NETN_MAX_WIDTH || D > 64 * NETN_KMAX || g_mlp3_route == 2;
}
bool mlp3_eligible(const NetArgs<float>& a) {
  if (!g_mlp3_route || a.loss != HTA_LOSS_REGRESSION) return false;
  if (!(a.mass_kind == HTA_MASS_NONE || a.mass_kind == HTA_MASS_DIAG)) return false;
  return mlp3_shape(a.n_layers, a.dims);
}

// The momentum workspace (see M3Chain::pw): one slot of 7 x 448 float4 per workgroup.  ABI 10: it is the CALLER's memory
// (hta_netn_hmc_workspace_bytes -> the `workspace` argument of hta_netn_hmc_sample / hta_netn_logp_grad); rounds 3-4 kept a
// hipMalloc'ed buffer per (device, stream) behind the ABI, grown with a hipStreamSynchronize + hipFree - an allocation and a
// synchronisation the boundary promises not to make, and a launch that could not be captured in a HIP graph.
static int mlp3_grid(int64_t C) {
  int cus = 256;
  int dev = 0;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  // one workgroup per CU is resident (151 KB of LDS); twice that many in the grid keeps the tail short, each workgroup walks
  // its chains in a grid-stride loop
  const int64_t gmax = 2 * (int64_t)cus;
  return (int)(C < gmax ? C : gmax);
}
static int64_t mlp3_slot_bytes(int grid) { return (int64_t)grid * 7 * M3_NT * 4 * (int64_t)sizeof(float); }
int64_t mlp3_workspace_bytes(int64_t C, int n_layers, const int* dims) {
  if (!dims || C <= 0 || !mlp3_shape(n_layers, dims)) return 0;
  return mlp3_slot_bytes(mlp3_grid(C));
}

template <int ACT> static int launch_mlp3(const NetArgs<float>& a, hipStream_t s) {
  static DevOnce done;
  const int NP = mlp3_data_np(a);
  const size_t lds = (mlp3_lds_floats() + (size_t)(a.dims[0] + 1) * NP) * sizeof(float);
  if (const int rc = allow_big_lds(done, "hta_netn_hmc (mlp3)", &mlp3_mfma_kernel<ACT>)) return rc;
  const int grid = mlp3_grid(a.C);
  const int64_t need = mlp3_slot_bytes(grid);
  HTA_REQUIRE(a.workspace && a.workspace_bytes >= need, "hta_netn_hmc (mlp3): workspace of %lld bytes required (hta_netn_hmc_workspace_bytes)",
              (long long)need);
  float* pws = static_cast<float*>(a.workspace);
  profile_begin(s);
  note_route("mlp3_mfma_kernel<%d>", ACT);
  mlp3_mfma_kernel<ACT><<<grid, M3_NT, lds, s>>>(a, NP, pws);
  profile_end(s);
  HTA_CHECK_LAUNCH("hta_netn_hmc (mlp3)");
  return HTA_OK;
}

int mlp3_mfma(const NetArgs<float>& a, hipStream_t s) {
  HTA_REQUIRE(a.theta && a.X && a.Y && a.C > 0, "hta_netn_hmc: NULL pointer / empty batch");
  HTA_REQUIRE(a.act >= 0 && a.act <= 2, "hta_netn_hmc: unknown activation %d", a.act);
  if (const int rc = check_split_args(a, "hta_netn_hmc", "hta_netn_logp_grad", "diagonal mass needs inv_mass and mass_factor")) return rc;
  if (a.act == 0) return launch_mlp3<0>(a, s);
  if (a.act == 1) return launch_mlp3<1>(a, s);
  return launch_mlp3<2>(a, s);
}

}  // namespace hta
