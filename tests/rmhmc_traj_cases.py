"""Cases for the trajectory-mode tests of the explicit-RMHMC kernels for Gaussian targets - rmhmc_fused_kernel<T,KH,1|2,tracked>,
rmhmc_fused_kernel_wide<56|64> (hamiltorch_amd/csrc/rmhmc_fused_chain_dev.hpp), rmhmc_mfma4_kernel, rmhmc_batch_kernel<25|28>
(rmhmc_fused_tiles_dev.hpp; all of them launched by rmhmc_fused.hip, after the draws of rmhmc_fused_momentum_dev.hpp), rmhmc_uv_kernel<G,
co|solo> (rmhmc_uv.hip), rmhmc_uvc_kernel and rmhmc_uvc2_kernel (rmhmc_uvc.hip) - and the driver that runs oracle/hmc_oracle.py on
them.  Plain numpy, no GPU, nothing of the library on the reference side.  Shared by tests/test_rmhmc_traj_cases_cpu.py (which checks
on the oracle alone that every case can tell a wrong kernel from a right one, and the launcher's rules restated here against the
table) and tests/test_gpu_rmhmc_traj.py (the kernels through hamiltorch_amd/_abi.py).  Same shape as tests/netn_traj_cases.py.

TARGET.  P = Q diag(linspace(.5, 2, D)) Q^T rounded to float32 (Q from numpy's QR of a seeded normal matrix), mean linspace(-1, 1, D),
log_norm = -1 - D / 4, starts mu + 0.3 z with z the Philox INIT normals of (seed, chain id), omega = 10, alpha = 1e6, chain offset 5,
8 trajectories, burn 2 unless the case says otherwise.  The REFERENCE is oracle/hmc_oracle.py:sample_rmhmc_explicit in float64 started
from those float32 numbers cast up, for the float32 and the float64 kernels alike.  Its momentum law follows
tests/test_gpu_rmhmc.py:oracle_momentum: "split" (chol(P) z1 + sqrt(jitter u) . z2) on the fused routes with jitter, "chol" without
jitter, with the tuning key rmhmc_momsplit = 0 and on the launch sequence (metric_eval_kernel) the refused D = 129 lands on.

LAUNCHER.  fused_plan, rmhmc_fused_sample's route conditions and the grid / group rules of hamiltorch_amd/csrc/rmhmc_fused.hip,
rmhmc_uv.hip and rmhmc_uvc.hip are restated below (fused_plan, expected_route, groups); the GPU tests hold them to the launcher through
_abi.last_route().  One thing the launcher does NOT have: a launch without pre-drawn momenta.  A workspace of exactly
rmhmc_workspace_bytes(C, D, 4, 0) makes rmhmc_sample lend the (unused) augmented-state area to the momentum kernels, four trajectories
per pass, so `block > 0` always and the in-kernel-Cholesky form (need_w) is reached through series = 0 alone.  The minimum workspace is
run all the same: two passes of four, the same bits as one pass of eight.

BOUNDS (the project's own; none is fitted to what a GPU returned).  Sample rows, `cur` and the reset row: float32 5e-4 max(1,
|want|.max()) with at most 5 % of the compared chains outside (1 of 31, 0 of 17, 11 and 9) - tests/test_gpu_rmhmc.py:
test_uvc_kernel_vs_oracle_at_cfg3, test_sample_rmhmc_vs_oracle; float64 1e-8, no chain outside.  H_old / H_new of trajectory 0 on
every chain: float32 2e-4 + 2e-5 |H| (the family's kernel-vs-kernel tests), float64 1e-9 max(1, |H|).  accept[T, C], reject_count and
acc_rate exact on every chain inside the row band.

STEP SIZES.  The explicit integrator accepts everything on this target up to eps ~ 1.8 and nothing from ~ 1.87; between them the
window in which the oracle alone rejects some proposals moves with D, L, the jitter and the seed.  Each case's (eps, seed) is the first
of eps = 1.820, 1.825 .. 1.865 x seed = base, base + 1, .. that meets every condition of tests/test_rmhmc_traj_cases_cpu.py; the
`tried` column counts the candidates that did not.  d97, d100, d112, d113, s100 and d129 (under its chol(G) z draw) met none of those 60 candidates with 9 chains and
L = 2 (wherever the oracle rejected at burn + 1, the rejecting chain had rejected trajectories 0 .. burn as well: no reset to see);
they were searched again with 11 chains (d129: 9 and 11) over eps = 1.8300, 1.8325 .. 1.8550 at L = 2 and 3; their `tried` counts that search.
Nothing else was looked at, and no GPU result entered the choice.

MEASURED when the tests were written (the tests print these figures again; nothing below is a bound).
Per case: oracle acceptance / chains rejecting at burn + 1 of the compared chains (k2: under the split law; its mom_* runs replay chol(G) z),
then per kernel, over every route that lands on it - one = rmhmc_fused_kernel<float,KH,1,*>, two = <float,KH,2>, wide, uv, uvc, uvc2,
mfma4, batch, f64 = rmhmc_fused_kernel<double,KH,1,false>, seq = the launch sequence (metric_eval_kernel) D = 129 lands on, mom_wave /
mom_wg = the one-chain kernel behind the wave and the workgroup momentum draw: the larger trajectory-0 energy error as a share of its
tolerance / the largest row or cur error of a chain inside the band as a share of the band / chains outside the band.
    k0    0.79 / 8 of 31:  uv 0.055/0.0027/0  one 0.065/0.0089/0  two 0.065/0.0089/0  uvc2 0.055/0.0027/0  mfma4 0.06/0.0093/0
            batch 0.065/0.0098/0
    k1    0.63 / 3 of 17:  uv 0.025/0.016/0  one 0.025/0.037/0  two 0.021/0.037/0  uvc2 0.025/0.016/0  mfma4 0.025/0.036/0
            batch 0.025/0.037/0
    k2    0.73 / 1 of 31:  uvc 0.026/0.016/0  one 0.027/0.037/0  two 0.016/0.037/0  uv 0.027/0.015/0  uvc2 0.027/0.015/0
            mfma4 0.029/0.037/0  batch 0.027/0.036/0  mom_wave 0.028/0.014/0  mom_wg 0.03/0.014/0
    k3    0.73 / 1 of 31:  uv 0.028/0.016/0  one 0.028/0.036/0  two 0.015/0.036/0  uvc2 0.028/0.016/0  mfma4 0.028/0.037/0
            batch 0.029/0.038/0
    w2    0.73 / 1 of 31:  one 0.018/0.04/0
    w5    0.76 / 7 of 31:  one 0.028/0.0081/0
    d1    0.63 / 16 of 31:  uvc 0.0019/0.0033/0  one 0.004/0.0023/0  two 0.004/0.0019/0  uv 0.0031/0.0023/0  uvc2 0.0031/0.0023/0
            mfma4 0.004/0.0023/0  batch 0.004/0.0023/0
    d3    0.72 / 6 of 31:  uvc 0.0048/0.0037/0  one 0.0054/0.0073/0  two 0.0054/0.0073/0  uv 0.0048/0.0021/0  uvc2 0.0048/0.0021/0
            mfma4 0.0071/0.0059/0  batch 0.0071/0.0059/0
    d7    0.74 / 5 of 31:  uvc 0.0078/0.014/0  one 0.0089/0.031/0  two 0.0067/0.031/0  uv 0.0089/0.017/0  uvc2 0.0089/0.017/0
            mfma4 0.0089/0.028/0  batch 0.0089/0.028/0  f64 1.3e-06/1.3e-05/0
    d32   0.85 / 1 of 31:  uvc 0.034/0.0034/0  one 0.034/0.0089/0  two 0.028/0.0089/0  uv 0.031/0.0033/0  uvc2 0.031/0.0033/0
            mfma4 0.034/0.0091/0  batch 0.032/0.009/0
    d33   0.80 / 8 of 31:  uvc 0.055/0.0027/0  one 0.06/0.0095/0  two 0.06/0.0095/0  uv 0.06/0.0028/0  uvc2 0.06/0.0028/0
            mfma4 0.065/0.01/0  batch 0.065/0.0099/0  f64 2e-06/6.6e-06/0
    d64   0.78 / 2 of 17:  uvc 0.065/0.0073/0  one 0.071/0.02/0  two 0.071/0.02/0  uv 0.065/0.0074/0  uvc2 0.065/0.0074/0
            mfma4 0.071/0.019/0  batch 0.074/0.019/0
    d97   0.67 / 5 of 11:  uvc 0.034/0.039/0  one 0.03/0.082/0  wide 0.03/0.082/0  two 0.025/0.082/0  uv 0.03/0.039/0
            uvc2 0.03/0.039/0  mfma4 0.03/0.082/0  batch 0.034/0.084/0
    d100  0.88 / 1 of 11:  uvc 0.033/0.0094/0  one 0.033/0.033/0  wide 0.033/0.033/0  two 0.033/0.033/0  uv 0.033/0.0098/0
            uvc2 0.033/0.0098/0  mfma4 0.037/0.032/0  batch 0.045/0.032/0  f64 1.7e-06/8.4e-06/0
    d101  0.79 / 2 of 9:  wide 0.053/0.037/0  one 0.053/0.037/0  two 0.053/0.037/0  batch 0.057/0.036/0
    d112  0.62 / 3 of 11:  wide 0.022/0.066/0  one 0.022/0.066/0  two 0.022/0.066/0  batch 0.022/0.069/0
    d113  0.89 / 1 of 11:  wide 0.031/0.026/0  one 0.031/0.026/0  two 0.031/0.026/0
    d128  0.76 / 3 of 9:  wide 0.027/0.03/0  one 0.027/0.03/0  two 0.027/0.03/0
    d129  0.57 / 1 of 9:  seq 0.081/0.056/0
    bm1   0.71 / 1 of 31:  uvc 0.0078/0.014/0  one 0.0089/0.031/0  two 0.0067/0.031/0  uv 0.0089/0.017/0  uvc2 0.0089/0.017/0
            mfma4 0.0089/0.028/0  batch 0.0089/0.028/0
    b0    0.71 / 2 of 31:  uvc 0.0078/0.014/0  one 0.0089/0.031/0  two 0.0067/0.031/0  uv 0.0089/0.017/0  uvc2 0.0089/0.017/0
            mfma4 0.0089/0.028/0  batch 0.0089/0.028/0
    b7    0.71 / - of 31:  uvc 0.0078/0.035/0  one 0.0089/0.076/0  two 0.0067/0.076/0  uv 0.0089/0.041/0  uvc2 0.0089/0.041/0
            mfma4 0.0089/0.068/0  batch 0.0089/0.068/0
    s7    0.75 / 6 of 31:  uv 0.0093/0.015/0  one 0.0089/0.027/0  two 0.0089/0.027/0  uvc2 0.0074/0.015/0  mfma4 0.009/0.03/0
            batch 0.009/0.03/0  f64 1.7e-06/1.8e-05/0
    s33   0.79 / 8 of 31:  uv 0.053/0.0028/0  one 0.058/0.0098/0  two 0.058/0.0098/0  uvc2 0.053/0.0028/0  mfma4 0.063/0.0092/0
            batch 0.063/0.0099/0  f64 1.7e-06/6.7e-06/0
    s100  0.89 / 1 of 11:  uv 0.038/0.0097/0  one 0.038/0.032/0  wide 0.038/0.032/0  two 0.037/0.032/0  uvc2 0.038/0.0097/0
            mfma4 0.038/0.032/0  batch 0.046/0.033/0  f64 5.9e-06/8.8e-06/0
Launch edges (17 chains each; 256 CUs):
    edge@256    0.74 / 4 on rmhmc_uvc_kernel<co>: 0.0098/0.0047/0
    edge@257    0.74 / 3 on rmhmc_uvc2_kernel<co>: 0.0077/0.003/0
    edge@513    0.72 / 2 on rmhmc_uvc2_kernel<co>: 0.0056/0.0058/0
    edge@1792   0.72 / 5 on rmhmc_uvc2_kernel<co>: 0.0048/0.0032/0
    edge@1793   0.69 / 5 on rmhmc_mfma4_kernel<true>: 0.0076/0.0043/0
    edge@8193   0.69 / 1 on rmhmc_fused_kernel<float,8,1,true>: 0.0043/0.004/0
    edge@32769  0.67 / 3 on rmhmc_mfma4_kernel<true>: 0.0076/0.0047/0
    edge@65537  0.68 / 4 on rmhmc_batch_kernel<25,true>: 0.0076/0.0022/0
Two launches cut at burn, burn + 1 and burn + 2, the padded allocation and the minimum workspace: the same bits as one plain launch on every
route run.  Before the hand-over fix in rmhmc_cols_dev.hpp (CHANGELOG): uvc2_co left 1 - 2 chains 0.6 - 3 away on d1, d3, d97, d100, s100 and
edge@257 (H_old of the trajectory after a partner-less reset: -1e8 .. -2e33), and d100 cut in two differed on uv1_co, uv2_solo and uvc2_co."""
import collections
import functools
import math

import numpy as np

import hmc_oracle as O

NTRAJ, BURN, CHAIN_OFFSET, OMEGA, ALPHA = 8, 2, 5, 10.0, 1e6
NOMINAL_CUS = 256          # MI355X; the GPU tests take the count from the device
QK, BATCH_D, FAMILY_D = 100, 112, 128          # rmhmc_fused.hip: QK, 16 BWV, fused_plan's D gate
GRID_ONE, GRID_MFMA4, GRID_BATCH = 8192, 8192, 4096          # workgroups: one- and two-chain kernels, mfma4 (4 chains each), batch (16)
GUARD = 1e-6               # float64 routes: no decision within GUARD max(1, |H|) of its threshold (tests/mlp_traj_cases.py)
ROW_TOL = {"f32": 5e-4, "f64": 1e-8}
MAX_OUTSIDE = {"f32": 0.05, "f64": 0.0}

Case = collections.namedtuple("Case", "id D C L jitter eps seed burn ntraj tried")


def _case(id, D, C, L, jitter, eps, seed, burn=BURN, tried=0):
    return Case(id, D, C, L, jitter, eps, seed, burn, NTRAJ, tried)


# id, D, chains, L, jitter, eps, seed
TABLE = [
    # refinement counts of the column kernels with series = 1: K = 0, 1, 2, 3
    _case("k0", 33, 31, 2, None, 1.84, 21, tried=4),
    _case("k1", 65, 17, 3, 6e-5, 1.825, 21, tried=1),
    _case("k2", 37, 31, 3, 1e-3, 1.82, 21),
    _case("k3", 37, 31, 3, 1.3e-3, 1.82, 21),
    # series = 0: the one-chain kernel factorises inside (need_w); K = 3 and 7
    _case("w2", 37, 31, 3, 2e-3, 1.82, 21),
    _case("w5", 31, 31, 2, 5e-2, 1.845, 21, tried=5),
    # D edges (jitter 1e-3: K = 2)
    _case("d1", 1, 31, 3, 1e-3, 1.82, 21),
    _case("d3", 3, 31, 3, 1e-3, 1.82, 21),
    _case("d7", 7, 31, 3, 1e-3, 1.82, 21),
    _case("d32", 32, 31, 2, 1e-3, 1.84, 21, tried=4),
    _case("d33", 33, 31, 2, 1e-3, 1.84, 21, tried=4),
    _case("d64", 64, 17, 2, 1e-3, 1.84, 21, tried=4),
    _case("d97", 97, 11, 3, 1e-3, 1.83, 21),
    _case("d100", 100, 11, 2, 1e-3, 1.84, 21, tried=4),
    _case("d101", 101, 9, 2, 1e-3, 1.84, 24, tried=34),
    _case("d112", 112, 11, 3, 1e-3, 1.83, 21),
    _case("d113", 113, 11, 2, 1e-3, 1.84, 21, tried=4),
    _case("d128", 128, 9, 2, 1e-3, 1.84, 22, tried=14),
    _case("d129", 129, 9, 3, 1e-3, 1.83, 21),
    # burn (d7 has burn 2)
    _case("bm1", 7, 31, 3, 1e-3, 1.82, 21, burn=-1),
    _case("b0", 7, 31, 3, 1e-3, 1.82, 21, burn=0),
    _case("b7", 7, 31, 3, 1e-3, 1.82, 21, burn=NTRAJ - 1),
    # jitter 1e-6: the series form of rmhmc_fused_kernel<double,...> (K = 2; in float32 K = 1)
    _case("s7", 7, 31, 3, 1e-6, 1.82, 21),
    _case("s33", 33, 31, 2, 1e-6, 1.84, 21, tried=4),
    _case("s100", 100, 11, 2, 1e-6, 1.84, 21, tried=4),
]
CASES = {c.id: c for c in TABLE}
F64_IDS = ("d7", "d33", "d100", "s7", "s33", "s100")          # jitter 1e-3: the Cholesky form in double; 1e-6: the series form
CUT_IDS = ("k2", "k0", "w2", "d100")                          # two launches over traj_offset
MOMENTUM_ID = "k2"                                            # the momentum kernels once each
ALL_CASES = dict(CASES)


def _register(case):
    ALL_CASES.setdefault(case.id, case)
    assert ALL_CASES[case.id] == case, (ALL_CASES[case.id], case)
    return case


# ---- the launch-edge runs: D = 3, 17 chains against the oracle ----
# C -> (eps, seed, tried) found at the nominal CU count; another C (another CU count) runs at the default
EDGE_STEPS = {256: (1.82, 31, 0), 257: (1.82, 31, 0), 513: (1.82, 31, 0), 1792: (1.82, 31, 0), 1793: (1.82, 31, 0), 8193: (1.825, 31, 1), 32769: (1.82, 31, 0), 65537: (1.82, 31, 0)}
EDGE_DEFAULT = (1.82, 31, 0)


def edge_case(C):
    eps, seed, tried = EDGE_STEPS.get(C, EDGE_DEFAULT)
    return _register(_case("edge@%d" % C, 3, C, 3, 1e-3, eps, seed, tried=tried))


def edge_sizes(cus):
    """name -> (C, the route keys that put it there): where rmhmc_uv_launch goes from one chain per workgroup to two, where the default
    route leaves the column kernels, and one chain past every grid cap."""
    return {"cus": (cus, "default"), "cus+1": (cus + 1, "default"), "2cus+1": (2 * cus + 1, "default"), "7cus": (7 * cus, "default"),
            "7cus+1": (7 * cus + 1, "default"), "one+1": (GRID_ONE + 1, "fused_t"), "mfma4+1": (4 * GRID_MFMA4 + 1, "mfma4_t"),
            "batch+1": (16 * GRID_BATCH + 1, "default")}


def edge_chains(C):
    """The 17 chains of a launch-edge run that go against the oracle: the first 4, the last 4 and 9 spread evenly between."""
    mid = np.round(np.linspace(4, C - 5, 11)[1:-1]).astype(np.int64)
    sel = np.concatenate([np.arange(4), mid, np.arange(C - 4, C)])
    assert sel.size == 17 and len(set(sel.tolist())) == 17
    return sel


# ---- the tuning keys of every route (tests/test_gpu_rmhmc_traj.py sets them, the launcher's rule restated below reads them) ----
DEFAULT_KEYS = {"rmhmc_fused": 1, "rmhmc_uv": 1, "rmhmc_uvc": 1, "rmhmc_uv_g": 0, "rmhmc_uv_co": 1, "rmhmc_mfma4": 1, "rmhmc_mfma4_lo": 1793,
                "rmhmc_mfma4_hi": 2049, "rmhmc_batch": 1, "rmhmc_pair": 1, "rmhmc_wide": 1, "rmhmc_momsplit": 1, "rmhmc_momwave": 1}
_ONE = {"rmhmc_uv": 0, "rmhmc_mfma4": 0, "rmhmc_batch": 0}
ROUTES = {
    "default": {},
    "fused_t": dict(_ONE, rmhmc_wide=0, rmhmc_pair=1),
    "fused_e": dict(_ONE, rmhmc_wide=0, rmhmc_pair=0),
    "wide_t": dict(_ONE, rmhmc_wide=1, rmhmc_pair=1),
    "wide_e": dict(_ONE, rmhmc_wide=1, rmhmc_pair=0),
    "pair2": dict(_ONE, rmhmc_wide=0, rmhmc_fused=3),
    "uv1_co": {"rmhmc_uv": 2, "rmhmc_uvc": 0, "rmhmc_uv_g": 1, "rmhmc_uv_co": 1},
    "uv1_solo": {"rmhmc_uv": 2, "rmhmc_uvc": 0, "rmhmc_uv_g": 1, "rmhmc_uv_co": 0},
    "uv2_co": {"rmhmc_uv": 2, "rmhmc_uvc": 0, "rmhmc_uv_g": 2, "rmhmc_uv_co": 1},
    "uv2_solo": {"rmhmc_uv": 2, "rmhmc_uvc": 0, "rmhmc_uv_g": 2, "rmhmc_uv_co": 0},
    "uvc_co": {"rmhmc_uv": 2, "rmhmc_uvc": 1, "rmhmc_uv_g": 1, "rmhmc_uv_co": 1},
    "uvc_solo": {"rmhmc_uv": 2, "rmhmc_uvc": 1, "rmhmc_uv_g": 1, "rmhmc_uv_co": 0},
    "uvc2_co": {"rmhmc_uv": 2, "rmhmc_uvc": 1, "rmhmc_uv_g": 2, "rmhmc_uv_co": 1},
    "uvc2_solo": {"rmhmc_uv": 2, "rmhmc_uvc": 1, "rmhmc_uv_g": 2, "rmhmc_uv_co": 0},
    "mfma4_t": {"rmhmc_mfma4": 2, "rmhmc_uv": 0, "rmhmc_pair": 1},
    "mfma4_e": {"rmhmc_mfma4": 2, "rmhmc_uv": 0, "rmhmc_pair": 0},
    "batch_t": {"rmhmc_batch": 2, "rmhmc_uv": 0, "rmhmc_mfma4": 0, "rmhmc_pair": 1},
    "batch_e": {"rmhmc_batch": 2, "rmhmc_uv": 0, "rmhmc_mfma4": 0, "rmhmc_pair": 0},
    "f64": {},
    # the momentum kernels behind the one-chain kernel: the wave draw and the workgroup draw (a factorisation per draw: "chol")
    "mom_wave": dict(_ONE, rmhmc_wide=0, rmhmc_momsplit=0, rmhmc_momwave=1),
    "mom_wg": dict(_ONE, rmhmc_wide=0, rmhmc_momsplit=0, rmhmc_momwave=0),
}
F32_ROUTES = tuple(r for r in ROUTES if r not in ("f64", "mom_wave", "mom_wg"))
# the kernel a route's keys ask for; expected_route() says where the launcher really sends a case (a refusal lands elsewhere)
ASKS_FOR = {"fused_t": "rmhmc_fused_kernel<float", "fused_e": "rmhmc_fused_kernel<float", "wide_t": "rmhmc_fused_kernel_wide", "wide_e": "rmhmc_fused_kernel_wide",
            "pair2": "rmhmc_fused_kernel<float", "uv1_co": "rmhmc_uv_kernel<1,co>", "uv1_solo": "rmhmc_uv_kernel<1,solo>", "uv2_co": "rmhmc_uv_kernel<2,co>",
            "uv2_solo": "rmhmc_uv_kernel<2,solo>", "uvc_co": "rmhmc_uvc_kernel<co>", "uvc_solo": "rmhmc_uvc_kernel<solo>", "uvc2_co": "rmhmc_uvc2_kernel<co>",
            "uvc2_solo": "rmhmc_uvc2_kernel<solo>", "mfma4_t": "rmhmc_mfma4_kernel<true>", "mfma4_e": "rmhmc_mfma4_kernel<false>",
            "batch_t": "rmhmc_batch_kernel", "batch_e": "rmhmc_batch_kernel", "f64": "rmhmc_fused_kernel<double",
            "mom_wave": "rmhmc_fused_kernel<float", "mom_wg": "rmhmc_fused_kernel<float"}


def tag(route):
    return "f64" if route == "f64" else "f32"


def momentum_law(case, route):
    """tests/test_gpu_rmhmc.py:oracle_momentum for a run of the family: "split" with jitter unless rmhmc_momsplit = 0, else "chol"."""
    keys = dict(DEFAULT_KEYS, **ROUTES[route])
    return "split" if (case.jitter is not None and keys["rmhmc_momsplit"]) else "chol"


def laws(case):
    """The momentum laws a case is run under (so the laws its step size has to discriminate under)."""
    if case.D > FAMILY_D:
        return ("chol",)          # D = 129 runs the launch sequence of rmhmc_explicit.hip (metric_eval_kernel): chol(G) z
    return ("split", "chol") if case.id == MOMENTUM_ID else (("chol",) if case.jitter is None else ("split",))


# ---- the launcher's rules, restated ----
def lam_min(D, f64=False):
    """The smallest eigenvalue of the case's P as the library's plan sees it (the spectrum in the state dtype)."""
    lam = np.linalg.eigvalsh(inputs_of(D)[0].astype(np.float64))
    return float(lam.min() if f64 else np.float32(lam.min()))


def fused_plan(D, jitter, f64=False, lmin=None, alpha=ALPHA):
    """hamiltorch_amd/csrc/rmhmc_fused.hip:fused_plan for a positive-definite spectrum: (K, series), K = -1: not in the family."""
    lmin = lam_min(D, f64) if lmin is None else lmin
    if D > FAMILY_D or not lmin > 0.0 or not alpha * lmin >= 20.0:
        return -1, 0
    if jitter is None:
        return 0, 1
    rho = jitter / lmin
    if rho > 0.25:
        return -1, 0
    if rho == 0.0:
        return 0, 1
    eps = 1.1e-16 if f64 else 6e-8
    series = int(D * rho ** 3 / 3.0 <= 0.25 * eps * (0.5 * D))
    K = max(1, int(math.ceil(math.log(eps * 0.25) / math.log(rho))) - 1)
    return (-1 if K > 40 else K), series


def kh(D):
    """The register slice of the one-chain kernel: half the contraction range, in eights."""
    return ((D + 1) // 2 + 7) // 8 * 8


def expected_route(case, route, cus=NOMINAL_CUS):
    """rmhmc_fused_sample's and rmhmc_uv_launch's conditions under the keys of `route`: the name _abi.last_route() must report, or
    None when the run leaves the family (fused_plan refuses).  `route`: a name of ROUTES, or the keys themselves (float32)."""
    k = dict(DEFAULT_KEYS, **(ROUTES[route] if isinstance(route, str) else route))
    f64 = route == "f64"
    D, C, jit = case.D, case.C, case.jitter is not None
    K, series = fused_plan(D, case.jitter, f64)
    if K < 0:
        return None
    lean = bool(series or not jit)                 # pre-drawn momenta are always there (see LAUNCHER above)
    T = "double" if f64 else "float"
    pair = k["rmhmc_fused"] == 3 and lean
    tf = "true" if k["rmhmc_pair"] else "false"
    if not f64:
        uv = (k["rmhmc_uv"] and k["rmhmc_mfma4"] != 2 and k["rmhmc_batch"] != 2 and not pair and lean and D <= QK
              and (C <= (7 if k["rmhmc_uv_co"] else 2) * cus or k["rmhmc_uv"] == 2))
        if uv:
            g = k["rmhmc_uv_g"] if k["rmhmc_uv_g"] in (1, 2) else (1 if C <= cus else 2)
            co = "co" if k["rmhmc_uv_co"] else "solo"
            if g == 1 and k["rmhmc_uvc"] and K == 2 and jit:
                return "rmhmc_uvc_kernel<%s>" % co
            if g == 2 and k["rmhmc_uvc"]:
                return "rmhmc_uvc2_kernel<%s>" % co
            return "rmhmc_uv_kernel<%d,%s>" % (g, co)
        if k["rmhmc_mfma4"] and not pair and lean and D <= QK and (k["rmhmc_mfma4_lo"] <= C < k["rmhmc_mfma4_hi"] or k["rmhmc_mfma4"] == 2):
            return "rmhmc_mfma4_kernel<%s>" % tf
        if k["rmhmc_batch"] and not pair and lean and D <= BATCH_D and (C >= 2048 or k["rmhmc_batch"] == 2):
            return "rmhmc_batch_kernel<%d,%s>" % (25 if D <= 100 else 28, tf)
    if pair:
        return "rmhmc_fused_kernel<%s,%d,2>" % (T, kh(D))
    if not f64 and k["rmhmc_wide"] and kh(D) in (56, 64) and C <= cus:
        return "rmhmc_fused_kernel_wide<%d,%s>" % (kh(D), tf)
    return "rmhmc_fused_kernel<%s,%d,1,%s>" % (T, kh(D), tf if not f64 else "false")


def groups(name, C):
    """(chains per workgroup, workgroups launched, chains of the last group) of the kernel `name` at C chains."""
    per = 16 if name.startswith("rmhmc_batch") else 4 if name.startswith("rmhmc_mfma4") else \
        2 if (name.startswith("rmhmc_uvc2") or name.startswith("rmhmc_uv_kernel<2") or name.endswith(",2>")) else 1
    cap = GRID_BATCH if per == 16 else GRID_ONE
    n = (C + per - 1) // per
    return per, min(n, cap), C - per * (n - 1)


def runs(cus=NOMINAL_CUS):
    """Every (case id, route) of the table: each float32 route on every case (the wide keys only where they change the instance, the
    momentum kernels on one case), the float64 route on F64_IDS.  A route that refuses a case is run all the same: expected_route says
    where it lands."""
    out = []
    for c in TABLE:
        for r in F32_ROUTES:
            if r.startswith("wide") and kh(c.D) not in (56, 64):
                continue
            out.append((c.id, r))
        if c.id in F64_IDS:
            out.append((c.id, "f64"))
        if c.id == MOMENTUM_ID:
            out += [(c.id, "mom_wave"), (c.id, "mom_wg")]
    return out


# ---- inputs and the oracle ----
def log_norm(D):
    return -1.0 - 0.25 * D


@functools.lru_cache(maxsize=None)
def inputs_of(D):
    """(P[D, D], mu[D]) in float32, read-only."""
    rng = np.random.default_rng(1000 + D)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    P = (Q * np.linspace(0.5, 2.0, D)) @ Q.T
    P = (0.5 * (P + P.T)).astype(np.float32)
    P = 0.5 * (P + P.T)
    mu = np.linspace(-1.0, 1.0, D).astype(np.float32)
    P.setflags(write=False); mu.setflags(write=False)
    return P, mu


def starts(case, chains=None):
    """theta_init of the chains `chains` (default: all) in float32: mu + 0.3 z, z the Philox INIT normals of (seed, chain id)."""
    chains = np.arange(case.C) if chains is None else np.asarray(chains)
    mu = inputs_of(case.D)[1].astype(np.float64)
    z = O.philox_normals(case.seed, CHAIN_OFFSET + chains, 0, case.D, O.PURPOSE_INIT, dtype=np.float64)
    return (mu + 0.3 * z).astype(np.float32)


class _Recording(O.GaussianTarget):
    """rm_hamiltonian asks for log p once: at a trajectory's start, then at its end."""

    def __init__(self, mu, P, log_norm):
        super().__init__(mu, P, log_norm)
        self.seen = []

    def logp(self, theta):
        self.seen.append(np.array(theta, copy=True))
        return super().logp(theta)


Ref = collections.namedtuple("Ref", "rows h_old h_new accept rejected acc_rate log_u starts cur theta0")


def run_oracle(case, law, chains=None, dtype=np.float64, mean="case", jitter="case", ntraj=None):
    """sample_rmhmc_explicit on the chains `chains` of the case (default: all), state and draws in `dtype`, from the float32 inputs.
    Ref: rows[T - burn, c, D] (row 0 = theta_init), h_old / h_new / accept[T, c], rejected[c], acc_rate[c], log_u[T, c] (float64),
    starts[T, c, D] (the point every trajectory starts from), cur[c, D] (the state after the last trajectory), theta0[c, D].
    mean=None: the target's mean at 0 (the starts stay); jitter=None: no jitter; ntraj: only the first trajectories."""
    P, mu = inputs_of(case.D)
    chains = np.arange(case.C) if chains is None else np.asarray(chains)
    ids = CHAIN_OFFSET + chains
    th0 = starts(case, chains)
    n = case.ntraj if ntraj is None else ntraj
    tg = _Recording((mu if mean == "case" else np.zeros_like(mu)).astype(dtype), P.astype(dtype), log_norm(case.D))
    ret, info = O.sample_rmhmc_explicit(tg, th0.astype(dtype), n, case.L, case.eps, OMEGA, ALPHA, min(case.burn, n - 1),
                                        case.jitter if jitter == "case" else jitter, O.PhiloxDraws(case.seed, ids, dtype), "softabs", momentum=law)
    assert len(tg.seen) == 2 * n
    acc = np.stack(info["accept"])
    ho, hn = np.stack(info["h_old"]), np.stack(info["h_new"])
    log_u = np.stack([np.log(O.PhiloxDraws(case.seed, ids, np.float64).mh_uniform(k).astype(np.float64)) for k in range(n)])
    begin = np.stack(tg.seen[0::2])
    # the state after the last trajectory: its proposal where it accepted, else where it started - or theta_init at burn + 1 (Q2)
    last = n - 1
    kept = th0.astype(dtype) if last == case.burn + 1 else begin[last]
    cur = np.where(acc[last][:, None], tg.seen[-1], kept)
    return Ref(np.stack(ret), ho, hn, acc, (~acc).sum(0), info["acc_rate"], log_u, begin, cur, th0)


def _frozen(ref):
    for a in ref:
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(cid, law):
    """The float64 oracle of a case under a momentum law, on all its chains - on the 17 of edge_chains for a launch-edge case;
    computed once per process, shared by every test that needs it, read-only."""
    case = ALL_CASES[cid]
    return _frozen(run_oracle(case, law, edge_chains(case.C) if cid.startswith("edge@") else None))


# ---- the bounds ----
def row_band(tag_, want):
    return ROW_TOL[tag_] * (max(1.0, float(np.abs(want).max())) if tag_ == "f32" else 1.0)


def h_tol(tag_, H):
    return 2e-4 + 2e-5 * np.abs(H) if tag_ == "f32" else 1e-9 * np.maximum(1.0, np.abs(H))


def max_outside(tag_, n_chains):
    """Chains allowed outside the row band: 5 % of the compared ones in float32 (1 of 31, 0 of 17, 11 and 9), none in float64."""
    return int(MAX_OUTSIDE[tag_] * n_chains)


def outside(rows, cur, ref, band):
    """Chain by chain: True where any entry of any row of the chain, or of the state handed back, is further than `band`."""
    assert rows.shape == ref.rows.shape and cur.shape == ref.cur.shape, (rows.shape, ref.rows.shape)
    with np.errstate(invalid="ignore"):
        return ~((np.abs(rows - ref.rows).max(axis=(0, 2)) <= band) & (np.abs(cur - ref.cur).max(axis=1) <= band))


def guard_margin(ref):
    """|min(0, H_old - H_new) - log u| / max(1, |H_old|, |H_new|): the distance of a Metropolis decision from its threshold."""
    scale = np.maximum(1.0, np.maximum(np.abs(ref.h_old), np.abs(ref.h_new)))
    return np.abs(np.minimum(0.0, ref.h_old - ref.h_new) - ref.log_u) / scale
