"""Cases of tests/test_gpu_scale.py (GPU) and tests/test_scale_cases.py (CPU): launches at the chain counts the published sweeps
run at, checked chain by chain on a PROBE SET.

Philox streams are keyed by the global chain id, so the oracle can reproduce any scattered subset of the chains of a launch without
simulating the others: `probe_ids(C)` names the chains a launch of C chains is checked on (a few hundred at most), the GPU result is
reduced to them on the device, the oracle runs on them only.

Plain module (numpy + the oracle, no torch): the same case list drives the GPU comparison and the CPU check that no case sits on a
borderline Metropolis decision.
"""
import numpy as np

import hmc_oracle as O

#: route thresholds of the dispatcher (csrc/hmc_gaussian.hip) and of samplers.py: the fused quad launch's limit, "quad_max_chains" /
#: the compiled kernels' published size, _CompiledHMC.PREDRAW_MAX_CHAINS, the 32-bit lane offsets' guard
EDGES = (4096, 65536, 131072, 1 << 20)
_FIXED = (0, 1, 15, 16, 63, 64, 255, 256, 1023, 1024)
N_RANDOM = 64


def probe_ids(C, edges=EDGES):
    """Sorted unique chain ids to check for a launch of C chains: the first lanes / waves / blocks, the last chains (C - 1, C - 2, C - 64,
    C - 65), both sides of every power of two from 2^12 up that is below C and of every route threshold in `edges`, and N_RANDOM ids
    drawn with a fixed seed - clipped to [0, C)."""
    C = int(C)
    ids = list(_FIXED) + [C - 1, C - 2, C - 64, C - 65]
    e = 1 << 12
    marks = []
    while e < C:
        marks.append(e)
        e <<= 1
    marks += [int(x) for x in edges]
    for m in marks:
        ids += [m - 1, m, m + 1]
    ids += [int(x) for x in np.random.default_rng(20241016).integers(0, C, N_RANDOM)]
    a = np.unique(np.asarray(ids, dtype=np.int64))
    return a[(a >= 0) & (a < C)]


def init_state(ids, D, scale):
    """Start of chain c, coordinate j: scale * (2 m / 65521 - 1) with m = (2654435761 c + 40503 j) mod 65521, evaluated in float64 (integer
    arithmetic exact in int64 up to 2^31 chains; one division, one multiplication, one subtraction and one scaling, each correctly rounded) -
    so that numpy on the probe ids and torch on the device for ALL chains produce the same bits without moving C x D values."""
    c = np.asarray(ids, dtype=np.int64)[:, None]
    j = np.arange(D, dtype=np.int64)[None, :]
    m = (c * 2654435761 + j * 40503) % 65521
    return ((m.astype(np.float64) * 2.0 / 65521.0) - 1.0) * float(scale)


SIGMA3 = np.array([[1.0, 0.6, 0.2], [0.6, 2.0, 0.5], [0.2, 0.5, 0.5]])      # BASELINE config 2's covariance (tests/test_gpu_hmc.py)


def rand_spd(D, seed, lo=0.5, hi=2.0):
    """tests/test_gpu_hmc.py::rand_spd"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    P = (Q * np.linspace(lo, hi, D)) @ Q.T
    return 0.5 * (P + P.T)


def gauss_model(D):
    """(precision, mean): config 2's target at D = 3, a random SPD precision (spectrum 0.5 ... 2) with a non-zero mean elsewhere"""
    if D == 3:
        return np.linalg.inv(SIGMA3), np.zeros(3)
    return rand_spd(D, 3), np.random.default_rng(D).standard_normal(D)


def num_rows(N, burn):
    return 1 + N - max(0, min(N, burn + 1))


Q3 = "hmc_gauss_quad_kernel<3,false,%d,7>"
EIG3 = "hmc_gauss_eig_kernel<float,3,false>"
SMALL = "hmc_gauss_small_kernel<float,%d,0,false,false>"

# One row per launch shape.  `abi`: the route the C ABI call takes with a workspace for `abi_chunk` trajectories per launch (all N when
# absent, "sample" = the count sample() derives from WS_CAP; `prepared`: hta_hmc_gaussian_prepare first, the fused launch needs it);
# `sample`: the route hamiltorch_amd.sample() takes - beyond _GaussianHMC.WS_CAP of look-ahead rows + one trajectory (C = 2^20 at W = 8, C = 2^22 at W = 4)
# sample() passes no workspace and the direct kernel draws in the lane: that is where the sweep's last point runs, the eigenbasis kernel at
# those sizes is reached through the ABI with a caller's workspace.  `tuning`: route keys set for the case (restored by the test).
# `off`: chain_offset of the call (the Philox key of chain c is off + c; one case crosses 2^31).  `seed`: chosen so that the oracle in fp32 and in fp64 take the same Metropolis decisions on the probe ids (tests/test_scale_cases.py).
GAUSS_CASES = [
    dict(id="fused-4096", C=4096, D=3, N=40, L=25, burn=3, eps=0.3, seed=11, prepared=True,
         abi="hmc_gauss_quad_fused_kernel<3,25>", sample="hmc_gauss_quad_fused_kernel<3,25>"),
    dict(id="past-fused-4104", C=4104, D=3, N=40, L=25, burn=3, eps=0.3, seed=12, abi=Q3 % 25, sample=Q3 % 25),
    dict(id="sweep-2^14", C=1 << 14, D=3, N=40, L=25, burn=-1, eps=0.3, seed=13, abi=Q3 % 25, sample=Q3 % 25),
    dict(id="sweep-2^16", C=1 << 16, D=3, N=40, L=25, burn=-1, eps=0.3, seed=14, off=(1 << 31) - 4096, abi=Q3 % 25, sample=Q3 % 25),
    dict(id="past-quad-65544", C=65544, D=3, N=12, L=25, burn=2, eps=0.3, seed=15, abi=EIG3, sample=EIG3),
    dict(id="sweep-2^18", C=1 << 18, D=3, N=10, L=25, burn=-1, eps=0.3, seed=16, off=1000003, abi=EIG3, sample=EIG3),
    dict(id="sweep-2^20", C=1 << 20, D=3, N=10, L=25, burn=-1, eps=0.3, seed=17, abi=EIG3, sample=EIG3),
    dict(id="sweep-2^22", C=1 << 22, D=3, N=10, L=25, burn=-1, eps=0.3, seed=18, abi=EIG3, sample=SMALL % 3),
    # the C <= 2^20 guard of the 32-bit lane offsets, "quad_max_chains" raised: widest record (D = 4: W = 8) and narrowest (D = 1)
    dict(id="guard-2^20-D4", C=1 << 20, D=4, N=12, L=10, burn=0, eps=0.25, seed=19, tuning={"quad_max_chains": 1 << 24},
         abi="hmc_gauss_quad_kernel<4,false,10,7>", sample=SMALL % 4),
    dict(id="guard-2^20+64-D4", C=(1 << 20) + 64, D=4, N=12, L=10, burn=0, eps=0.25, seed=20, tuning={"quad_max_chains": 1 << 24},
         abi="hmc_gauss_quad_kernel<4,false,10>", sample=SMALL % 4),
    dict(id="guard-2^20-D1", C=1 << 20, D=1, N=12, L=10, burn=0, eps=0.25, seed=21, tuning={"quad_max_chains": 1 << 24},
         abi="hmc_gauss_quad_kernel<1,false,10,7>", sample="hmc_gauss_quad_kernel<1,false,10,7>"),
    dict(id="guard-2^20+64-D1", C=(1 << 20) + 64, D=1, N=12, L=10, burn=0, eps=0.25, seed=22, tuning={"quad_max_chains": 1 << 24},
         abi="hmc_gauss_quad_kernel<1,false,10>", sample="hmc_gauss_quad_kernel<1,false,10>"),
    # host chunking by WS_CAP: 600 trajectories of 32 768 chains are 251 + 251 + 98 at the 128 MiB cap (the test reads the cap from samplers.py)
    dict(id="ws-cap-chunks", C=1 << 15, D=3, N=600, L=5, burn=5, eps=0.3, seed=23, abi_chunk="sample",
         abi=Q3 % 5, sample=Q3 % 5, min_launches=2),
    # wave-per-chain grid of 131 072 workgroups
    dict(id="wave-2^17-D64", C=1 << 17, D=64, N=6, L=5, burn=0, eps=0.25, seed=24,
         abi="hmc_gauss_wave_eig_kernel<float,1>", sample="hmc_gauss_wave_eig_kernel<float,1>"),
]

# rows past element 2^31 and byte 2^33 of the sample tensor: 514 rows of 2^20 chains x 4 coordinates (8.6 GB of fp32)
BIG_CASE = dict(id="rows-past-2^31", C=1 << 20, D=4, N=513, L=5, burn=-1, eps=0.25, seed=25, abi_chunk=57,
                abi="hmc_gauss_eig_kernel<float,4,false>", sample=SMALL % 4)


def gauss_start(case, ids):
    return init_state(ids, case["D"], 0.5)


def gauss_oracle(case, ids, dtype=np.float32):
    """(rows, info) of oracle.sample_hmc for the chains `ids` of the case, arithmetic in `dtype` (the start is the fp32 one either way)"""
    P, mu = gauss_model(case["D"])
    th0 = gauss_start(case, ids).astype(np.float32).astype(dtype)
    tgt = O.GaussianTarget(mu.astype(dtype), P.astype(dtype), 0.0)
    return O.sample_hmc(tgt, th0, case["N"], case["L"], case["eps"], case["burn"], None, O.PhiloxDraws(case["seed"], case.get("off", 0) + np.asarray(ids), dtype))


# ---- compiled callbacks ------------------------------------------------------------------------------------------------------------
# tests/test_gpu_jit.py's funnel (funnel_device / oracle.FunnelTarget), D = 11; the start keeps |v| <= 0.25 so that no chain begins in the
# funnel's neck, where fp32 rounding is amplified along a trajectory (test_compiled_funnel_vs_oracle allows a tenth of its chains
# outside the band for that reason; here the cap is two chains, so the instance stays where fp32 and fp64 agree - checked on the CPU:
# at a step of 0.05 the ORACLE in fp32 leaves the 2e-4 band of the oracle in fp64 on a few probe chains of 8 x 25 steps, at 0.03 the
# two stay within 1e-5 for every seed tried)
CB_D = 11
CB_HMC_CASES = [
    dict(id="cb-hmc-2^16", C=1 << 16, N=8, L=25, burn=-1, eps=0.03, seed=31),
    dict(id="cb-hmc-2^17+64", C=(1 << 17) + 64, N=8, L=25, burn=-1, eps=0.03, seed=32),
]
CB_CAP_CASE = dict(id="cb-hmc-predraw-cap", C=1 << 16, N=100, L=4, burn=3, eps=0.05, seed=33)      # 42 + 42 + 16 trajectories under PREDRAW_CAP
CB_SCALE = 0.25


def cb_start(case, ids, D=CB_D):
    return init_state(ids, D, CB_SCALE)


def cb_hmc_oracle(case, ids, dtype):
    th0 = cb_start(case, ids).astype(np.float32).astype(dtype)        # (every start is an fp32 value, whatever the run's type)
    return O.sample_hmc(O.FunnelTarget(CB_D), th0, case["N"], case["L"], case["eps"], case["burn"], None,
                        O.PhiloxDraws(case["seed"], np.asarray(ids), dtype))


# tests/test_gpu_jit_split.py's logistic list (D = 6, M = 3) at its own step size
SPLIT_CASES = [
    dict(id="cb-split-symmetric", C=1 << 16, N=8, L=8, burn=0, eps=0.1, seed=41, kind="symmetric"),
    dict(id="cb-split-rand", C=1 << 16, N=8, L=8, burn=0, eps=0.1, seed=42, kind="rand"),
]
SPLIT_D, SPLIT_SCALE = 6, 0.5


def split_oracle(case, ids, dtype, logistic_oracle):
    """`logistic_oracle`: tests/test_gpu_jit_split.py::logistic_oracle as a function of the numpy dtype -> (logp_fns, grad_fns)"""
    lf, gf = logistic_oracle(dtype)
    th0 = init_state(ids, SPLIT_D, SPLIT_SCALE).astype(np.float32).astype(dtype)
    return O.sample_hmc(None, th0, case["N"], case["L"], case["eps"], case["burn"], None, O.PhiloxDraws(case["seed"], np.asarray(ids), dtype),
                        grad_fns=gf, logp_fns=lf, split_kind=case["kind"])


# the funnel RMHMC case of tests/test_gpu_jit.py::test_fused_rmhmc_kernel_vs_oracle (D = 11, jitter 1e-3, alpha = 1, burn = -1)
RMHMC_CASES = [
    dict(id="cb-rmhmc-2^16-f32", C=1 << 16, N=3, L=3, burn=-1, eps=0.08, omega=10.0, alpha=1.0, jitter=1e-3, seed=51, dtype="f32"),
    dict(id="cb-rmhmc-4096-f64", C=4096, N=3, L=3, burn=-1, eps=0.08, omega=10.0, alpha=1.0, jitter=1e-3, seed=52, dtype="f64"),
]
RMHMC_SCALE = 0.25


def rmhmc_oracle(case, ids, dtype):
    th0 = init_state(ids, CB_D, RMHMC_SCALE).astype(np.float32).astype(dtype)
    with np.errstate(all="ignore"):
        return O.sample_rmhmc_explicit(O.FunnelTarget(CB_D, np.ones(CB_D - 1)), th0, case["N"], case["L"], case["eps"], case["omega"],
                                       case["alpha"], case["burn"], case["jitter"], O.PhiloxDraws(case["seed"], np.asarray(ids), dtype))


def allowed_share(n_probe):
    """Share of the probe chains that may leave the band (a Metropolis decision within rounding of its threshold): 0.5 % of them and never
    more than 2 chains - with fewer than 200 probe chains that is none."""
    return min(0.005, 2.0 / n_probe)
