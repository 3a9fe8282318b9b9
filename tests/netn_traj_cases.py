"""Cases for the trajectory-mode tests of the deep-net sampler kernels - netn_hmc_kernel<T,PB,WV> (hamiltorch_amd/csrc/netn_hmc.hip:
1 .. 4 Linear layers, Gaussian / Bernoulli / softmax likelihoods) and mlp3_mfma_kernel<ACT> (hamiltorch_amd/csrc/mlp3_mfma.hip: two
wide hidden layers on the matrix cores) - and the driver that runs oracle/hmc_oracle.py on them.  Plain numpy, no GPU.  Shared by
tests/test_netn_traj_cases_cpu.py (which checks on the oracle alone that every case can tell a wrong kernel from a right one) and
tests/test_gpu_netn_traj.py (the kernels through hamiltorch_amd/_abi.py).  Same shape as tests/mlp_traj_cases.py.

Every table case: C = 32 chains, L = 3 steps, 7 trajectories, burn = 1, taus = [1 + 0.25 k], prior_scale = M (what
define_split_model_log_prob hands the kernel), tau_out = 6, chain offset 3.  X ~ N(0, 1) in float32 from the case's generator; Y by
likelihood: regression sin(sum_k x_k) + 0.1 N(0, 1) per output, softmax integer labels in [0, O) stored as floats (shape [N], as
the ABI takes them), Bernoulli 0 / 1 per output.  theta0 = 0.3 x the Philox INIT normals in float32; the diagonal inverse mass is
0.5 + rng.random(D) rounded to float32.  The REFERENCE is oracle/hmc_oracle.py:MLPRegressionTarget in float64 started from those
float32 numbers cast up, for the float32 and the float64 kernels alike - so one oracle run serves every route of a case.

BOUNDS (the project's own; none is fitted to what a GPU returned).  Energies of trajectory 0: 3e-4 max(1, |H|.max()) in float32 and
1e-10 max(1, ...) in float64 - what test_netn_logp_grad_vs_oracle allows the same kernel's log-probability (test_mlp3_logp_grad_vs_
oracle: 1e-4; 3e-4 here as well, the energy adds the kinetic term).  Sample rows chain by chain: 5e-4 with at most 7 % of the
compared chains outside in float32 (2 of 32; 1 of the 17 chains of a launch-edge run), 1e-9 with no chain outside in float64.  The
step sizes and seeds below were chosen on the CPU so that the conditions of tests/test_netn_traj_cases_cpu.py hold.

MEASURED when the tests were written (the tests print these figures again; nothing below is a bound).  Oracle, float64: acceptance
over the compared chains x trajectories / chains rejecting at burn + 1.  MI355X: the larger trajectory-0 energy error as a share of
its tolerance / chains outside the sample band, per route (w2, w4: tuning key netn_waves = 2, 4).
    id    eps     seed  oracle      f32         f64         w2          w4
    n1    2e-2    201   0.78 / 10   5e-4 / 0    3e-6 / 0
    n2    2.8e-2  202   0.43 /  8   5e-4 / 0    4e-6 / 0                            (3e-2: a float64 decision 5e-7 from its threshold)
    n3    1e-1    203   0.70 / 12   5e-4 / 0    3e-6 / 0
    n4    5e-2    204   0.80 /  4   4e-4 / 0    4e-6 / 0    4e-6 / 0    4e-6 / 0    (the wave variants in float64)
    n5    2e-2    205   0.57 / 14   4e-4 / 0
    n6    3e-2    206   0.69 / 11   3e-4 / 0    2e-6 / 0
    n7    1.2e-1  207   0.69 /  8   6e-4 / 0                                        (8e-2: 0.88 / 2, one reset visible; 1e-1: 0.75 / 6)
    n8    1e-1    208   0.70 / 12   4e-4 / 0                                        (1.2e-1: 0.64 / 9; 1.5e-1: 0.04 / 32)
    n9    1.8e-2  239   0.62 / 23   3e-4 / 0                4e-4 / 0    5e-4 / 0    (seed 209: 0.90 .. 0.96 at 1.2e-2 .. 2e-2, too many accepts)
    n10   = n1 to the bit in float32 and in float64
    w1    7e-2    211   0.76 /  9   4e-4 / 0    (mlp3_mfma_kernel<1>; 3e-2 .. 4e-2 accept 0.96 .. 0.98)
    w2    2e-2    212   0.76 /  7   2e-4 / 0    (mlp3_mfma_kernel<0>)
    w3    3e-2    213   0.60 / 15   7e-4 / 0    (mlp3_mfma_kernel<2>; 2e-2 accepts 0.92, 4e-2 0.12)
    w4    5e-2    214   0.54 / 16   4e-4 / 0    (mlp3_mfma_kernel<0>)
    res        3e-2    221   0.51 / 10 of 17 at C = 256 on <float,4,1>, 0.53 / 9 of 17 at C = 257 on <float,2,1>: 4e-4 / 0 on both
    grid_netn  0.2     222   0.81 /  7 of 17 (65537 chains): 5e-4 / 0
    grid_mlp3  1.2e-1  223   0.69 /  5 of 17 (513 chains): 3e-4 / 0
The float32-state oracle leaves the band on no chain of any case.  The largest float32 sample difference on a chain inside the band
is 3.7e-6 (n7), at most 1.1e-6 elsewhere; float64: 1.1e-15.  Trajectory-0 energies of two / four waves against one wave: within 4.9e-4
on n9 (|H| up to 3.4e3; allowed 2.05), 4.6e-13 on n4 in float64 (allowed 2.4e-7)."""
import collections
import functools

import numpy as np

import hmc_oracle as O

C, L, NTRAJ, BURN, CHAIN_OFFSET = 32, 3, 7, 1, 3
TAU_OUT = 6.0
ACT_ID = {"relu": 0, "tanh": 1, "sigmoid": 2}
LOSS_NAME = {"regression": "regression", "softmax": "multi_class_linear_output", "bernoulli": "binary_class_linear_output"}
ENERGY_TOL = {"f32": 3e-4, "f64": 1e-10}
SAMPLE_TOL = {"f32": 5e-4, "f64": 1e-9}
MAX_OUTSIDE = {"f32": 0.07, "f64": 0.0}
KINK_TOL, KINK_MAX_CHAINS = 5e-4, 1           # float32-state oracle against the float64 oracle: at most one chain further apart
# float64 routes: no Metropolis decision within GUARD max(1, |H|) of its threshold.  The float64 kernel is allowed 1e-10 max(1, |H|) on
# each of the two energies of a decision; 1e-6 is 5000 times their sum, so no decision the kernel may legitimately get can flip and no
# chain needs an exemption (tests/mlp_traj_cases.py: GUARD).
GUARD = 1e-6

# integ: "symmetric" (SPLITTING, S:499-540) | "kmid" | "rand" | "leapfrog" (M = 1, S:281-302)
Case = collections.namedtuple("Case", "id dims act loss Nb M integ mass eps seed tau_out extra_rows C L ntraj")


def _case(id, dims, act, loss, Nb, M, integ, mass, eps, seed, tau_out=TAU_OUT, extra_rows=0, C=C, L=L, ntraj=NTRAJ):
    return Case(id, tuple(dims), act, loss, Nb, M, integ, mass, eps, seed, tau_out, extra_rows, C, L, ntraj)


NETN_CASES = [
    _case("n1", (1, 10, 10, 1), "relu", "regression", 100, 4, "symmetric", "diag", 2e-2, 201),
    _case("n2", (4, 3), "relu", "softmax", 50, 3, "rand", "none", 2.8e-2, 202),
    _case("n3", (3, 8, 8, 8, 2), "sigmoid", "bernoulli", 35, 2, "kmid", "diag", 1e-1, 203),
    _case("n4", (5, 7, 6, 3), "tanh", "softmax", 130, 1, "leapfrog", "diag", 5e-2, 204),
    _case("n5", (64, 5, 1), "relu", "regression", 65, 2, "symmetric", "diag", 2e-2, 205),
    _case("n6", (6, 17, 18, 1), "tanh", "regression", 24, 3, "symmetric", "diag", 3e-2, 206),
    _case("n7", (2, 3, 10), "tanh", "softmax", 33, 2, "symmetric", "none", 1.2e-1, 207),
    _case("n8", (6, 1), "relu", "bernoulli", 64, 2, "kmid", "diag", 1e-1, 208),
    _case("n9", (3, 5, 2), "tanh", "regression", 300, 2, "rand", "diag", 1.8e-2, 239),
    # n1 with five more rows of X and Y, all 1e6, behind the M Nb rows the splits use: the same numbers to the bit
    _case("n10", (1, 10, 10, 1), "relu", "regression", 100, 4, "symmetric", "diag", 2e-2, 201, extra_rows=5),
]
MLP3_CASES = [
    _case("w1", (2, 65, 3, 1), "tanh", "regression", 24, 3, "symmetric", "diag", 7e-2, 211),
    _case("w2", (4, 5, 66, 1), "relu", "regression", 50, 2, "kmid", "diag", 2e-2, 212),
    _case("w3", (3, 104, 4, 1), "sigmoid", "regression", 230, 1, "leapfrog", "diag", 3e-2, 213),
    _case("w4", (1, 65, 2, 1), "relu", "regression", 16, 4, "rand", "none", 5e-2, 214),
]
CASES = {c.id: c for c in NETN_CASES + MLP3_CASES}
NETN_IDS = tuple("n%d" % k for k in range(1, 10))
F64_IDS = ("n1", "n2", "n3", "n4", "n6")
MLP3_IDS = ("w1", "w2", "w3", "w4")
# (route, case id): "f32" = float32 as dispatched, "f64" = float64, "mlp3" = float32 on mlp3_mfma_kernel
RUNS = [("f32", i) for i in NETN_IDS] + [("f64", i) for i in F64_IDS] + [("mlp3", i) for i in MLP3_IDS]
# tuning key netn_waves = 2 / 4: n9 in float32, n4 in float64
WAVE_RUNS = [("w2", "n9"), ("w4", "n9"), ("w2", "n4"), ("w4", "n4")]
WAVES = {"f32": 1, "f64": 1, "w2": 2, "w4": 4}

# ---- the launch-edge runs: 17 chains against the oracle (grid_chains) ----
GRID_NETN = 65536          # netn_hmc's cap on workgroups
NOMINAL_CUS = 256          # MI355X; the GPU tests take the count from the device


def res_case(C):
    """One workgroup of <float,4,1> fits per CU (83528 bytes of LDS): C = CUs keeps PB = 4, C = CUs + 1 drops to PB = 2."""
    return _register(_case("res@%d" % C, (3, 16, 16, 2), "tanh", "regression", 140, 2, "symmetric", "diag", 3e-2, 221, C=C, L=2, ntraj=4))


def grid_netn_case():
    return _register(_case("grid_netn", (1, 2, 1), "relu", "regression", 4, 2, "symmetric", "diag", 0.2, 222, C=GRID_NETN + 1, L=2, ntraj=4))


def grid_mlp3_case(C):
    """mlp3's grid is 2 CUs: C = 2 CUs + 1 gives workgroup 0 a second chain in its momentum slot of the workspace."""
    return _register(_case("grid_mlp3@%d" % C, (1, 65, 1, 1), "relu", "regression", 8, 2, "symmetric", "diag", 1.2e-1, 223, C=C, L=2, ntraj=4))


ALL_CASES = dict(CASES)


def _register(case):
    ALL_CASES.setdefault(case.id, case)
    assert ALL_CASES[case.id] == case
    return case


def tag(route, cid):
    """The precision of a run: "f32" or "f64"."""
    if route in ("w2", "w4"):
        return "f64" if cid == "n4" else "f32"
    return "f64" if route == "f64" else "f32"


# netn_hmc_kernel<T,PB,WV> per (route, id); the CPU tests hold the table to the launcher's rule restated
NETN_PB = {"n1": 2, "n2": 1, "n3": 1, "n4": 4, "n5": 2, "n6": 1, "n7": 1, "n8": 1, "n9": 4, "n10": 2, "grid_netn": 1}
WAVE_PB_WV = {("w2", "n9"): (4, 2), ("w4", "n9"): (2, 4), ("w2", "n4"): (2, 2), ("w4", "n4"): (1, 4)}


def expected_route(route, cid):
    case = ALL_CASES[cid]
    if route == "mlp3":
        return "mlp3_mfma_kernel<%d>" % ACT_ID[case.act]
    T = "double" if tag(route, cid) == "f64" else "float"
    if route in ("w2", "w4"):
        return "netn_hmc_kernel<%s,%d,%d>" % ((T,) + WAVE_PB_WV[route, cid])
    return "netn_hmc_kernel<%s,%d,1>" % (T, NETN_PB[cid])


def lds_for(dims, pb, wv, itemsize=4):
    """hamiltorch_amd/csrc/netn_hmc.hip: netn_hmc's lds_for, restated."""
    D, SW = n_params(dims), sum(dims)
    Dp = (D + 63) // 64 * 64
    return (2 * Dp + 4 + wv * 2 * (SW + 2) * (64 * pb + 1)) * itemsize + 64 * 4


def resident(dims, pb, wv, cus, itemsize=4):
    """... and its resident(): workgroups the chip holds at once (150 KB of LDS and 32 waves per CU)."""
    return cus * min((150 * 1024) // lds_for(dims, pb, wv, itemsize), 32 // wv)


def launcher_rule(dims, Nb, C, waves, cus, itemsize=4):
    """(PB, WV) as netn_hmc picks them: halve WV while Nb <= 32 WV, then PB from 4 while Nb <= 32 PB WV - or while the chains of the
    launch would not all be resident."""
    wv, pb = (4 if waves >= 4 else 2 if waves >= 2 else 1), 4
    while wv > 1 and (Nb <= 32 * wv or resident(dims, 1, wv, cus, itemsize) < C):
        wv //= 2
    while pb > 1 and (Nb <= 32 * pb * wv or resident(dims, pb, wv, cus, itemsize) < C):
        pb //= 2
    return pb, wv


def n_blocks(dims):
    """4 x 4 blocks of the matrix-core gradient: per layer ceil(O / 4) x ceil((I + 1) / 4) (weights | bias)."""
    return sum(((dims[l + 1] + 3) // 4) * ((dims[l] + 4) // 4) for l in range(len(dims) - 1))


def n_params(case_or_dims):
    dims = getattr(case_or_dims, "dims", case_or_dims)
    return sum(dims[l] * dims[l + 1] + dims[l + 1] for l in range(len(dims) - 1))


def n_rows(case):
    return case.ntraj - BURN          # params_init and one row per trajectory n > burn


def taus(case):
    return [1.0 + 0.25 * k for k in range(2 * (len(case.dims) - 1))]


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """(X[N, n_in], Y[N, O] - [N] for softmax -, theta0[C, D], inv_mass[D] or None) in float32; N = M Nb + extra_rows."""
    case = ALL_CASES[cid]
    rng = np.random.default_rng(case.seed)
    n, n_in, n_out = case.M * case.Nb, case.dims[0], case.dims[-1]
    X = rng.standard_normal((n, n_in)).astype(np.float32)
    if case.loss == "softmax":
        Y = rng.integers(0, n_out, n).astype(np.float32)
    elif case.loss == "bernoulli":
        Y = rng.integers(0, 2, (n, n_out)).astype(np.float32)
    else:
        Y = (np.sin(X.sum(1))[:, None] + 0.1 * rng.standard_normal((n, n_out))).astype(np.float32)
    D = n_params(case)
    im = (0.5 + rng.random(D)).astype(np.float32) if case.mass == "diag" else None
    if case.extra_rows:
        X = np.concatenate([X, np.full((case.extra_rows, n_in), 1e6, np.float32)])
        Y = np.concatenate([Y, np.full((case.extra_rows,) + Y.shape[1:], 1e6, np.float32)])
    th0 = (0.3 * O.philox_normals(case.seed, np.arange(case.C), 0, D, O.PURPOSE_INIT, dtype=np.float64)).astype(np.float32)
    for a in (X, Y, th0) + (() if im is None else (im,)):
        a.setflags(write=False)
    return X, Y, th0, im


def targets(case):
    """One oracle target per split over its Nb rows of the case's data (rows beyond M Nb belong to no split)."""
    X, Y = inputs(case.id)[:2]
    return [O.MLPRegressionTarget(list(case.dims), X[m * case.Nb:(m + 1) * case.Nb], Y[m * case.Nb:(m + 1) * case.Nb], taus(case), case.tau_out,
                                  float(case.M), case.act, loss=LOSS_NAME[case.loss]) for m in range(case.M)]


Ref = collections.namedtuple("Ref", "samples h_old h_new accept rejected log_u starts")


def run_oracle(case, chains=None, dtype=np.float64, chain_offset=CHAIN_OFFSET, mass="case"):
    """oracle/hmc_oracle.py:sample_hmc on the rows `chains` of the case (default: all), state and draws in `dtype`, from the float32
    inputs.  Ref: samples[rows, c, D], h_old / h_new / accept[ntraj, c], rejected[c], log_u[ntraj, c] (float64), starts[ntraj, c, D]
    (the point every trajectory starts from).  mass=None: the same run without the case's diagonal mass."""
    X, Y, th0, im = inputs(case.id)
    if mass is None:
        im = None
    chains = np.arange(case.C) if chains is None else np.asarray(chains)
    ids = chain_offset + chains
    tg = targets(case)
    assert (case.integ == "leapfrog") == (case.M == 1)
    draws = O.PhiloxDraws(case.seed, ids, dtype=dtype)
    mass = None if im is None else im.astype(dtype)
    start = th0[chains].astype(dtype)
    seen = []                                     # hmc_hamiltonian asks the first closure for log p at a trajectory's start, then at its end

    def first_logp(theta):
        seen.append(theta.copy())
        return tg[0].logp(theta)

    if case.integ == "leapfrog":
        proxy = collections.namedtuple("Proxy", "logp grad")(first_logp, tg[0].grad)
        ret, info = O.sample_hmc(proxy, start, case.ntraj, case.L, case.eps, BURN, mass, draws)
    else:
        ret, info = O.sample_hmc(None, start, case.ntraj, case.L, case.eps, BURN, mass, draws, grad_fns=[t.grad for t in tg],
                                 logp_fns=[first_logp] + [t.logp for t in tg[1:]], split_kind=case.integ)
    assert len(seen) == 2 * case.ntraj
    acc = np.stack(info["accept"])
    log_u = np.stack([np.log(O.PhiloxDraws(case.seed, ids, dtype=np.float64).mh_uniform(k)) for k in range(case.ntraj)])
    return Ref(np.stack(ret), np.stack(info["h_old"]), np.stack(info["h_new"]), acc, (~acc).sum(0), log_u, np.stack(seen[0::2]))


def _frozen(ref):
    for a in ref:
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(cid):
    """The float64 oracle of a table case, computed once per process and shared by every test that needs it; read-only."""
    return _frozen(run_oracle(CASES[cid]))


def grid_chains(case):
    """The chains of a launch-edge run that go against the oracle: the first 8 and the last 9 (in a grid-stride run the last one is
    workgroup 0's second chain)."""
    return np.concatenate([np.arange(8), np.arange(case.C - 9, case.C)])


@functools.lru_cache(maxsize=None)
def grid_reference(cid):
    case = ALL_CASES[cid]
    return _frozen(run_oracle(case, grid_chains(case)))


def outside(got, want, tol):
    """tests/test_gpu_netn.py:_cmp's rule, chain by chain: True where any entry of any row of the chain is further than tol."""
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.abs(got - want).max(axis=(0, 2)) > tol


def max_outside(tag_, n_chains):
    """Chains allowed outside the sample band: 7 % of the compared ones in float32 (2 of 32, 1 of 17), none in float64."""
    return int(MAX_OUTSIDE[tag_] * n_chains)


def guard_margin(ref):
    """|H_old - H_new - log u| / max(1, |H_old|, |H_new|) per trajectory and chain: the distance of a Metropolis decision from its
    threshold, relative to the energies it is formed from."""
    scale = np.maximum(1.0, np.maximum(np.abs(ref.h_old), np.abs(ref.h_new)))
    return np.abs(ref.h_old - ref.h_new - ref.log_u) / scale
