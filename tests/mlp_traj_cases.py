"""Cases for the trajectory-mode tests of the one-hidden-layer MLP sampler kernels (csrc/mlp_mfma_dev.hpp, csrc/mlp_hmc.hip) and the
driver that runs oracle/hmc_oracle.py on them.  Plain numpy, no GPU.  Shared by tests/test_mlp_traj_cases_cpu.py (which checks on
the oracle alone that every case can tell a wrong kernel from a right one) and tests/test_gpu_mlp_traj.py (the kernels through
hamiltorch_amd/_abi.py).

Every case: C = 32 chains, L = 3 steps, 7 trajectories, burn = 1, tau = [1, 1.5, 2, 2.5], prior_scale = M (what
define_split_model_log_prob hands the kernel), chain offset 3.  X ~ N(0, 1), Y = sin(sum_k x_k) + 0.1 N(0, 1) in float32 from the
case's generator; theta0 = 0.3 x the Philox INIT normals in float32; the diagonal inverse mass is 0.5 + rng.random(D) rounded to
float32.  The REFERENCE is the oracle in float64 started from those float32 numbers cast up, for the float32 and the float64
kernels alike - so one oracle run serves every route of a case.

BOUNDS (none is fitted to what a GPU returned).  Energies of trajectory 0: 3e-4 max(1, |H|.max()) in float32 and 1e-10 max(1, ...)
in float64 - what test_native_logp_grad_vs_oracle allows the same kernels' log-probability.  Sample rows chain by chain: 5e-4 with
at most 7 % of the chains outside in float32 (tests/test_gpu_mlp.py:_cmp), 1e-9 with no chain outside in float64.  The step sizes
and seeds below were chosen on the CPU so that the conditions of tests/test_mlp_traj_cases_cpu.py hold.

MEASURED when the tests were written (the tests print these figures again; nothing below is a bound).  Oracle, float64: acceptance
over 32 chains x 7 trajectories / chains rejecting at burn + 1.  MI355X: the larger trajectory-0 energy error as a share of its
tolerance / chains outside the sample band, per route.
    id   eps      oracle      mfma          valu          f64
    m1   3e-2     0.49 / 15   4e-4 / 0      4e-4 / 0      3e-6 / 0
    m2   3e-2     0.50 / 19   9e-4 / 0
    m3   3e-2     0.74 /  8   5e-4 / 0
    m4   2e-2     0.54 / 15   2e-3 / 1      3e-4 / 1      3e-6 / 0     (the float32-state oracle leaves the band on one chain as well)
    m5   2e-2     0.59 / 15   3e-4 / 0
    m6   6e-2     0.49 / 16   7e-4 / 0      1e-3 / 0
    m7   2e-3     0.66 /  9   3e-4 / 0
    m8   3e-2     0.69 /  6   5e-4 / 0
    m9   3e-2     0.49 / 15   = m1 to the bit on both float32 routes
    v1   3e-2     0.64 / 15                 2e-4 / 0      3e-6 / 0
    v2   3e-3     0.50 / 19                 3e-4 / 0
    v3   1.58e-2  0.67 / 18                 8e-4 / 0      4e-6 / 0     (1.5e-2 accepts 0.96, 1.7e-2 0.04: the stability edge)
    v4   2e-3     0.80 / 10                 3e-4 / 0
    grid 0.2      0.54 / 10 of 17 (8193 chains), 0.44 / 9 of 17 (4097): 3e-4 / 0 on both kernels
The largest float32 sample difference on a chain inside the band is 3.7e-5 (m7), 2e-6 elsewhere; float64: 8e-16."""
import collections
import functools

import numpy as np

import hmc_oracle as O

C, L, NTRAJ, BURN, CHAIN_OFFSET = 32, 3, 7, 1, 3
TAU = (1.0, 1.5, 2.0, 2.5)
ACT_ID = {"relu": 0, "tanh": 1, "sigmoid": 2}
ENERGY_TOL = {"f32": 3e-4, "f64": 1e-10}
SAMPLE_TOL = {"f32": 5e-4, "f64": 1e-9}
MAX_OUTSIDE = {"f32": 0.07, "f64": 0.0}
KINK_TOL, KINK_MAX_CHAINS = 5e-4, 1           # float32-state oracle against the float64 oracle: at most one chain further apart
# float64 cases: no Metropolis decision within GUARD max(1, |H|) of its threshold.  The float64 kernel is allowed 1e-10 max(1, |H|) on
# each of the two energies of a decision; 1e-6 is 5000 times their sum, so no decision the kernel may legitimately get can flip and no
# chain needs an exemption.  (1e-3 max(1, |H|) cannot be met by any seed or step size: |H| is 8e2 .. 1e4 on these shapes, the band is
# 1 .. 10 energy units wide on either side, and it holds 12 .. 110 of a case's 224 decisions.)
GUARD = 1e-6

# integ: "symmetric" (SPLITTING, S:499-540) | "kmid" | "rand" | "leapfrog" (M = 1, S:281-302)
Case = collections.namedtuple("Case", "id n_in H act Nb M integ mass eps seed tau_out extra_rows C L ntraj")


def _case(id, n_in, H, act, Nb, M, integ, mass, eps, seed, tau_out=6.0, extra_rows=0, C=C, L=L, ntraj=NTRAJ):
    return Case(id, n_in, H, act, Nb, M, integ, mass, eps, seed, tau_out, extra_rows, C, L, ntraj)


CASES = {c.id: c for c in [
    _case("m1", 4, 17, "tanh", 24, 3, "symmetric", "diag", 3e-2, 101),
    _case("m2", 5, 48, "relu", 40, 2, "kmid", "diag", 3e-2, 102),
    _case("m3", 12, 40, "sigmoid", 72, 2, "rand", "none", 3e-2, 103),
    _case("m4", 16, 33, "relu", 150, 2, "symmetric", "diag", 2e-2, 104),
    _case("m5", 9, 130, "tanh", 36, 2, "symmetric", "diag", 2e-2, 105),
    _case("m6", 2, 16, "relu", 50, 1, "leapfrog", "diag", 6e-2, 106),
    _case("m7", 8, 100, "relu", 100, 4, "symmetric", "diag", 2e-3, 107, tau_out=100.0),
    _case("m8", 1, 256, "tanh", 16, 2, "rand", "diag", 3e-2, 108),
    # m1 with five more rows of X and Y, all 1e6, behind the M Nb rows the splits use: the same numbers to the bit
    _case("m9", 4, 17, "tanh", 24, 3, "symmetric", "diag", 3e-2, 101, extra_rows=5),
    _case("v1", 4, 65, "tanh", 24, 3, "symmetric", "diag", 3e-2, 111),
    _case("v2", 17, 600, "relu", 20, 2, "symmetric", "diag", 3e-3, 112),
    _case("v3", 32, 130, "sigmoid", 36, 2, "kmid", "diag", 1.58e-2, 113),
    _case("v4", 8, 300, "relu", 300, 2, "rand", "none", 2e-3, 114),
]}

# the grid-stride runs: Linear(1, 3)-ReLU-Linear(3, 1), 4 x 2 points, one chain more than the launch has workgroups
GRID = {"mfma": 8192, "valu": 4096}
GRID_CASES = {k: _case("grid_" + k, 1, 3, "relu", 4, 2, "symmetric", "diag", 0.2, 121, C=g + 1, L=2, ntraj=4) for k, g in GRID.items()}

# through sample_split_model / sample_model (chain offset 0): Linear(4, 33)-Tanh-Linear(33, 1) with the diagonal mass
API_CASES = {"split": _case("api_split", 4, 33, "tanh", 8, 3, "symmetric", "diag", 3e-2, 131),
             "full": _case("api_full", 4, 33, "tanh", 24, 1, "leapfrog", "diag", 6e-2, 132)}
ALL_CASES = dict(CASES, **{c.id: c for c in list(GRID_CASES.values()) + list(API_CASES.values())})

MFMA_ROUTE = {"m1": "mlp_mfma_kernel<1,2,1,512>", "m2": "mlp_mfma_kernel<2,3,0,512>", "m3": "mlp_mfma_kernel<3,5,2,512>",
              "m4": "mlp_mfma_kernel<4,8,0,512>", "m5": "mlp_mfma_kernel<3,8,1,1024>", "m6": "mlp_mfma_kernel<1,4,0,512>",
              "m7": "mlp_mfma_kernel<2,7,0,512>", "m8": "mlp_mfma_kernel<1,8,1,1024>", "m9": "mlp_mfma_kernel<1,2,1,512>",
              "grid_mfma": "mlp_mfma_kernel<1,1,0,512>"}
# mlp1_hmc_kernel<T,INMAX,NT,ACT,EXACT>
VALU_ROUTE = {"m1": "mlp1_hmc_kernel<%s,4,512,1,true>", "m4": "mlp1_hmc_kernel<%s,16,512,0,true>", "m6": "mlp1_hmc_kernel<%s,4,512,0,false>",
              "v1": "mlp1_hmc_kernel<%s,4,512,1,true>", "v2": "mlp1_hmc_kernel<%s,32,1024,0,false>",
              "v3": "mlp1_hmc_kernel<%s,32,512,2,true>", "v4": "mlp1_hmc_kernel<%s,8,512,0,true>", "m9": "mlp1_hmc_kernel<%s,4,512,1,true>",
              "grid_valu": "mlp1_hmc_kernel<%s,4,512,0,false>"}

MFMA_IDS = ("m1", "m2", "m3", "m4", "m5", "m6", "m7", "m8")
VALU_IDS = ("m1", "m4", "m6", "v1", "v2", "v3", "v4")
F64_IDS = ("m1", "m4", "v1", "v3")
# (route, case id): route "mfma" = float32 as dispatched, "valu" = float32 with tuning key mlp_valu, "f64" = float64
RUNS = [("mfma", i) for i in MFMA_IDS] + [("valu", i) for i in VALU_IDS] + [("f64", i) for i in F64_IDS]


def expected_route(route, cid):
    if route == "mfma":
        return MFMA_ROUTE[cid]
    return VALU_ROUTE[cid] % ("double" if route == "f64" else "float")


def n_params(case):
    return case.H * case.n_in + 2 * case.H + 1


def n_rows(case):
    return case.ntraj - BURN          # params_init and one row per trajectory n > burn


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """(X[N, n_in], Y[N], theta0[C, D], inv_mass[D] or None) in float32; N = M Nb + extra_rows."""
    case = ALL_CASES[cid]
    rng = np.random.default_rng(case.seed)
    n = case.M * case.Nb
    X = rng.standard_normal((n, case.n_in)).astype(np.float32)
    Y = (np.sin(X.sum(1)) + 0.1 * rng.standard_normal(n)).astype(np.float32)
    D = n_params(case)
    im = (0.5 + rng.random(D)).astype(np.float32) if case.mass == "diag" else None
    if case.extra_rows:
        X = np.concatenate([X, np.full((case.extra_rows, case.n_in), 1e6, np.float32)])
        Y = np.concatenate([Y, np.full(case.extra_rows, 1e6, np.float32)])
    th0 = (0.3 * O.philox_normals(case.seed, np.arange(case.C), 0, D, O.PURPOSE_INIT, dtype=np.float64)).astype(np.float32)
    for a in (X, Y, th0) + (() if im is None else (im,)):
        a.setflags(write=False)
    return X, Y, th0, im


class Target(O.MLPRegressionTarget):
    """oracle/hmc_oracle.py:MLPRegressionTarget for one hidden layer, one output and the Gaussian likelihood with its five einsum
    contractions written as np.matmul and no backward pass where only the value is asked for: the same formulas line by line
    (prior, unpacking and activation are the parent's own), three times faster at H = 300, Nb = 300, where the parent takes 0.2 s
    per call and a run makes over a hundred calls.  The CPU tests hold it to the parent's value and gradient at 1e-12 on every
    case."""

    def _forward(self, theta):
        dt = theta.dtype
        assert len(self.dims) == 3 and self.dims[-1] == 1 and self.loss == "regression"
        X, Y = self.X.astype(dt), self.Y.astype(dt)
        (W1, b1), (W2, b2) = self._unpack(theta)                     # [C, H, in], [C, H], [C, 1, H], [C, 1]
        z = np.matmul(X, W1.transpose(0, 2, 1))                      # [C, N, H]
        z += b1[:, None, :]
        h, dh = self._act(z)
        r = np.matmul(h, W2.transpose(0, 2, 1)) + b2[:, None, :] - Y[None]                 # [C, N, 1]
        ll = (-0.5 * dt.type(self.tau_out) * np.sum(r * r, axis=1)).sum(axis=-1)
        return X, W2, h, dh, r, ll

    def logp(self, theta):
        theta = np.atleast_2d(theta)
        return (self._forward(theta)[-1] + self._prior(theta)[0]).astype(theta.dtype)

    def logp_and_grad(self, theta):
        theta = np.atleast_2d(theta)
        dt = theta.dtype
        X, W2, h, dh, r, ll = self._forward(theta)
        delta = -dt.type(self.tau_out) * r
        lp_prior, g = self._prior(theta)
        d1 = delta * W2                                                                      # [C, N, H]
        d1 *= dh
        parts = [np.matmul(d1.transpose(0, 2, 1), X).reshape(theta.shape[0], -1), d1.sum(axis=1),
                 np.matmul(delta.transpose(0, 2, 1), h)[:, 0, :], delta.sum(axis=1)]
        return (ll + lp_prior).astype(dt), g + np.concatenate(parts, axis=1)


def targets(case, cls=Target):
    """One target per split over its Nb rows of the case's data (rows beyond M Nb belong to no split)."""
    X, Y = inputs(case.id)[:2]
    return [cls([case.n_in, case.H, 1], X[m * case.Nb:(m + 1) * case.Nb], Y[m * case.Nb:(m + 1) * case.Nb], TAU, case.tau_out,
                float(case.M), case.act) for m in range(case.M)]


Ref = collections.namedtuple("Ref", "samples h_old h_new accept rejected log_u")


def run_oracle(case, chains=None, dtype=np.float64, chain_offset=CHAIN_OFFSET):
    """oracle/hmc_oracle.py:sample_hmc on the rows `chains` of the case (default: all), state and draws in `dtype`, from the float32
    inputs.  Ref: samples[rows, c, D], h_old / h_new / accept[ntraj, c], rejected[c], log_u[ntraj, c] (float64)."""
    X, Y, th0, im = inputs(case.id)
    chains = np.arange(case.C) if chains is None else np.asarray(chains)
    ids = chain_offset + chains
    tg = targets(case)
    assert (case.integ == "leapfrog") == (case.M == 1)
    draws = O.PhiloxDraws(case.seed, ids, dtype=dtype)
    mass = None if im is None else im.astype(dtype)
    start = th0[chains].astype(dtype)
    if case.integ == "leapfrog":
        ret, info = O.sample_hmc(tg[0], start, case.ntraj, case.L, case.eps, BURN, mass, draws)
    else:
        ret, info = O.sample_hmc(None, start, case.ntraj, case.L, case.eps, BURN, mass, draws, grad_fns=[t.grad for t in tg],
                                 logp_fns=[t.logp for t in tg], split_kind=case.integ)
    acc = np.stack(info["accept"])
    log_u = np.stack([np.log(O.PhiloxDraws(case.seed, ids, dtype=np.float64).mh_uniform(k)) for k in range(case.ntraj)])
    return Ref(np.stack(ret), np.stack(info["h_old"]), np.stack(info["h_new"]), acc, (~acc).sum(0), log_u)


@functools.lru_cache(maxsize=None)
def reference(cid):
    """The float64 oracle of a table case, computed once per process and shared by every test that needs it; read-only."""
    ref = run_oracle(CASES[cid])
    for a in ref:
        a.setflags(write=False)
    return ref


def grid_chains(case):
    """The chains of a grid-stride run that go against the oracle: the first 8 and the last 9 (the last one is the workgroup's
    second chain)."""
    return np.concatenate([np.arange(8), np.arange(case.C - 9, case.C)])


@functools.lru_cache(maxsize=None)
def grid_reference(kind):
    case = GRID_CASES[kind]
    ref = run_oracle(case, grid_chains(case))
    for a in ref:
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def api_reference(kind):
    ref = run_oracle(API_CASES[kind], chain_offset=0)
    for a in ref:
        a.setflags(write=False)
    return ref


def outside(got, want, tol):
    """tests/test_gpu_mlp.py:_cmp's rule, chain by chain: True where any entry of any row of the chain is further than tol."""
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.abs(got - want).max(axis=(0, 2)) > tol


def guard_margin(ref):
    """|H_old - H_new - log u| / max(1, |H_old|, |H_new|) per trajectory and chain: the distance of a Metropolis decision from its
    threshold, relative to the energies it is formed from."""
    scale = np.maximum(1.0, np.maximum(np.abs(ref.h_old), np.abs(ref.h_new)))
    return np.abs(ref.h_old - ref.h_new - ref.log_u) / scale
