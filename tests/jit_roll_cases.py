"""Likelihoods summed over data rows for the tests of the rolled callback route (hamiltorch_amd/jit/roll.py): plain closures over
tensors, synthetic data from a fixed generator.  Shared by tests/test_jit_roll_cpu.py and tests/test_gpu_jit_roll.py.

Every case has an ORACLE TARGET next to it: a numpy class with batched `logp(theta)` / `grad(theta)` in closed form, written from the
mathematics and built from the callable's own `f.data` (`oracle_target(f)`), in the shape oracle/hmc_oracle.py:sample_hmc expects.  The
arithmetic follows theta's dtype (a float32 theta gives the target evaluated in float32), and every sum over data rows is numpy's
pairwise sum over a contiguous last axis - no BLAS call, so the float32 figures do not depend on the BLAS at hand.  `RUNS` are the
sampler runs the GPU tests compare with the oracle chain by chain; the CPU test file runs the float32 oracle against the float64
oracle on each of them."""
import math

import numpy as np
import torch

import hmc_oracle as O


def _t(a, dtype, device):
    return torch.tensor(np.asarray(a), dtype=dtype, device=device)


def logistic(N=40, D=3, dtype=torch.float64, device="cpu", seed=0):
    """Case 1: Bayesian logistic regression, binary labels - (y log s(Xw) + (1 - y) log s(-Xw)).sum() - 0.5 |w|^2."""
    rng = np.random.default_rng(seed)
    X, y = _t(rng.standard_normal((N, D)), dtype, device), _t((rng.uniform(size=N) > 0.5).astype(np.float64), dtype, device)

    def f(w):
        z = X @ w
        return (y * torch.log(torch.sigmoid(z)) + (1 - y) * torch.log(torch.sigmoid(-z))).sum() - 0.5 * (w * w).sum()
    f.data, f.target = (X, y), LogisticTarget
    return f


def hierarchical(N=24, D=4, dtype=torch.float64, device="cpu", seed=1):
    """Case 2: linear regression with a sampled noise scale - sigma = exp(th[D-1]), Normal(X b, sigma).log_prob(y).sum()."""
    rng = np.random.default_rng(seed)
    X, y = _t(rng.standard_normal((N, D - 1)), dtype, device), _t(rng.standard_normal(N), dtype, device)

    def f(th):
        sigma = torch.exp(th[D - 1])
        return torch.distributions.Normal(X @ th[:D - 1], sigma).log_prob(y).sum()
    f.data, f.target = (X, y), HierarchicalTarget
    return f


def two_structures(n=16, D=3, dtype=torch.float64, device="cpu", seed=2, n_gauss=None):
    """Case 3: n Poisson rows (log rate Xp w) + n_gauss Gaussian rows (mean Xg w, unit scale; n of them unless given) + a Gaussian
    prior; the LAST Poisson row has x = 0 features, folds to a constant of another shape and stays in the rest."""
    rng = np.random.default_rng(seed)
    m = n if n_gauss is None else n_gauss
    Xp = rng.standard_normal((n + 1, D)) * 0.5
    Xp[n] = 0.0
    k = rng.poisson(2.0, n + 1).astype(np.float64)
    Xp, k = _t(Xp, dtype, device), _t(k, dtype, device)
    Xg, yg = _t(rng.standard_normal((m, D)), dtype, device), _t(rng.standard_normal(m), dtype, device)

    def f(w):
        eta = Xp @ w
        r = yg - Xg @ w
        return (k * eta - torch.exp(eta)).sum() - 0.5 * (r * r).sum() - 0.25 * (w * w).sum()
    f.data, f.target = (Xp, k, Xg, yg), TwoStructuresTarget
    return f


def big_logistic(N=1500, D=4, dtype=torch.float64, device="cpu", seed=3):
    """A data set beyond straight-line code (value + gradient: ~45 000 scalar operations, limit 6000): y z - softplus(z), prior."""
    rng = np.random.default_rng(seed)
    X, y = _t(rng.standard_normal((N, D)), dtype, device), _t((rng.uniform(size=N) > 0.5).astype(np.float64), dtype, device)

    def f(w):
        z = X @ w
        return (y * z - torch.nn.functional.softplus(z)).sum() - 0.5 * (w * w).sum()
    f.data, f.target = (X, y), BigLogisticTarget
    return f


# ---- oracle targets: the same densities in closed form, numpy, batched over chains ---------------------------------------------------
HL2P = 0.5 * math.log(2.0 * math.pi)


def _dot(th, X):
    """th[..., D] . X[N, D] -> [..., N], every product summed over D in index order."""
    return (th[..., None, :] * X).sum(-1)


def _back(r, X):
    """sum over rows of r[..., N] X[N, D] -> [..., D]: numpy's pairwise sum over the N contiguous elements of each (chain, feature)."""
    return np.ascontiguousarray(r[..., None, :] * X.T).sum(-1)


class _Target:
    def __init__(self, *data, stored=np.float64):
        """`stored`: the dtype the data are held in on the device (float32 data are rounded once, whatever the arithmetic)."""
        self.data = [np.asarray(d.detach().cpu().numpy() if isinstance(d, torch.Tensor) else d, dtype=np.float64).astype(stored).astype(np.float64)
                     for d in data]

    def _data(self, th):
        return [d.astype(th.dtype) for d in self.data]


class LogisticTarget(_Target):
    """sum_i [y_i log s(z_i) + (1 - y_i) log s(-z_i)] - |w|^2 / 2, z = X w;  log s(z) = -log(1 + e^-z);  d/dz = y - s(z)."""

    def logp(self, th):
        X, y = self._data(th)
        z = _dot(th, X)
        return (-(y * np.logaddexp(0, -z) + (1 - y) * np.logaddexp(0, z))).sum(-1) - 0.5 * (th * th).sum(-1)

    def grad(self, th):
        X, y = self._data(th)
        return _back(y - 1 / (1 + np.exp(-_dot(th, X))), X) - th


class BigLogisticTarget(LogisticTarget):
    """The same density as its callable writes it: sum_i [y_i z_i - log(1 + e^z_i)] - |w|^2 / 2."""

    def logp(self, th):
        X, y = self._data(th)
        z = _dot(th, X)
        return (y * z - np.logaddexp(0, z)).sum(-1) - 0.5 * (th * th).sum(-1)


class HierarchicalTarget(_Target):
    """sum_i log N(y_i; x_i . b, e^t) with th = (b, t):  -e^-2t |r|^2 / 2 - N t - N log sqrt(2 pi), r = y - X b."""

    def _parts(self, th):
        X, y = self._data(th)
        r = y - _dot(th[..., :-1], X)
        return X, r, np.exp(-2 * th[..., -1]), (r * r).sum(-1)

    def logp(self, th):
        X, r, e, ss = self._parts(th)
        return -0.5 * e * ss - X.shape[0] * th[..., -1] - X.shape[0] * HL2P

    def grad(self, th):
        X, r, e, ss = self._parts(th)
        return np.concatenate([e[..., None] * _back(r, X), (e * ss - X.shape[0])[..., None]], -1).astype(th.dtype)


class TwoStructuresTarget(_Target):
    """sum_i [k_i eta_i - e^eta_i] - |yg - Xg w|^2 / 2 - |w|^2 / 4, eta = Xp w (the row with x = 0 contributes the constant -1)."""

    def logp(self, th):
        Xp, k, Xg, yg = self._data(th)
        eta, r = _dot(th, Xp), yg - _dot(th, Xg)
        return (k * eta - np.exp(eta)).sum(-1) - 0.5 * (r * r).sum(-1) - 0.25 * (th * th).sum(-1)

    def grad(self, th):
        Xp, k, Xg, yg = self._data(th)
        return _back(k - np.exp(_dot(th, Xp)), Xp) + _back(yg - _dot(th, Xg), Xg) - 0.5 * th


def oracle_target(f, stored=np.float64):
    """The numpy target of a callable made by one of the builders above, from the same data."""
    return f.target(*f.data, stored=stored)


# ---- the runs of tests/test_gpu_jit_roll.py that are compared with oracle.sample_hmc ---------------------------------------------------
NP = {torch.float32: np.float32, torch.float64: np.float64}
TOL = {torch.float64: 1e-9, torch.float32: 2e-4}       # tests/test_gpu_jit.py: compiled against the oracle, chain by chain
MAX_FLIPPED = 0.03                                     # share of chains that may leave the band (a flipped accept decision)


def rand_spd(D, seed, lo=0.5, hi=1.5):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    P = (Q * np.linspace(lo, hi, D)) @ Q.T
    return 0.5 * (P + P.T)


def masses(D, dtype):
    """tests/test_gpu_jit.py:masses."""
    rng = np.random.default_rng(0)
    return {"none": None, "diag": rng.uniform(0.5, 2.0, D).astype(NP[dtype]), "full": rand_spd(D, 7).astype(NP[dtype])}


class _Upcast:
    """The float32 draws handed to float64 arithmetic: the same numbers, no rounding of their own."""

    def __init__(self, draws):
        self.draws = draws

    def normals(self, n, D, sub=0):
        return self.draws.normals(n, D, sub).astype(np.float64)

    def mh_uniform(self, n):
        return self.draws.mh_uniform(n).astype(np.float64)


class Run:
    """One sampler run on one case: the callable, its oracle target, start, mass matrix and the oracle's result (computed once)."""

    def __init__(self, case, D, eps, C=130, samples=10, L=5, burn=0, mass="none", seed=11, off=3, scale=0.3, **data):
        self.case, self.D, self.eps, self.C, self.samples, self.L, self.burn, self.mass = case, D, eps, C, samples, L, burn, mass
        self.seed, self.off, self.scale, self.data = seed, off, scale, data
        self._oracle = {}

    def fn(self, dtype=torch.float64, device="cpu"):
        return globals()[self.case](dtype=dtype, device=device, **self.data)

    def start(self, dtype):
        z = O.philox_normals(self.seed, self.off + np.arange(self.C), 0, self.D, O.PURPOSE_INIT, dtype=np.float64)
        return (self.scale * z).astype(NP[dtype])

    def inv_mass(self, dtype):
        return masses(self.D, dtype)[self.mass]

    def kwargs(self):
        """What sample() takes besides the callable, the start and inv_mass."""
        return dict(num_samples=self.samples, num_steps_per_sample=self.L, step_size=self.eps, burn=self.burn, seed=self.seed,
                    chain_offset=self.off, debug=2, verbose=False)

    def oracle(self, dtype, exact=False):
        """oracle.sample_hmc on the Philox draws of (seed, chain offset) in `dtype` -> (rows [n, C, D], info).  exact=True: float64
        arithmetic on the start, mass matrix, draws and (float32) data of the float32 run - that run without its rounding."""
        key = (dtype, exact)
        if key not in self._oracle:
            draws = O.PhiloxDraws(self.seed, self.off + np.arange(self.C), NP[dtype])
            th0, im = self.start(dtype), self.inv_mass(dtype)
            if exact:
                assert dtype == torch.float32
                draws, th0, im = _Upcast(draws), th0.astype(np.float64), None if im is None else im.astype(np.float64)
            ref, info = O.sample_hmc(oracle_target(self.fn(), NP[dtype]), th0, self.samples, self.L, self.eps, self.burn, im, draws)
            ref = np.stack(ref)
            assert ref.dtype == (np.float64 if exact else NP[dtype])
            self._oracle[key] = (ref, info)
        return self._oracle[key]


def edge_eps(rows):
    """A step size at which about one proposal in ten is rejected: the posterior scale of the unit prior (curvature 1) with at most a
    quarter per row from the likelihood."""
    return round(1.0 / math.sqrt(1.0 + rows / 4.0), 3)


# rows over waves: (rows, W) with a short last wave, a wave of exactly one row, waves with r0 == rows and r0 > rows, W > rows; 8 rows is
# the fewest from which roll.py forms a group (ROLL_MIN_ROWS) - the pairs below that need the rule lowered in the test
EDGE_PAIRS = {torch.float64: [(41, 4), (13, 2), (5, 4), (9, 8), (3, 8), (8, 8)], torch.float32: [(17, 16), (40, 16), (9, 8), (8, 16)]}
MASS_ROWS = [("none", 0), ("diag", 3), ("full", -1)]           # mass kind, burn: spread as in test_compiled_funnel_vs_oracle
RUNS = {"two_structures": Run("two_structures", 3, 0.2, C=96, scale=0.2, n=7, n_gauss=19),
        "lds_logistic_1": Run("logistic", 3, edge_eps(200), C=70, N=200),          # tile 85: 85 + 85 + 30 rows on one wave
        "lds_logistic_2": Run("logistic", 3, edge_eps(250), C=70, N=250),          # 125 rows per wave at W = 2: 85 + 40
        "lds_hierarchical": Run("hierarchical", 4, 0.055, C=70, scale=0.2, N=300),   # U = 1, 4 slots: tile 96, 96 + 96 + 96 + 12
        "mass_hierarchical": Run("hierarchical", 4, 0.15, C=96, scale=0.2, mass="full", burn=3),
        "chunks": Run("logistic", 3, edge_eps(41), C=70, samples=12, burn=2, mass="diag", N=41),
        "long": Run("big_logistic", 4, 0.06, C=130, samples=8, L=5, scale=0.1)}
for _rows in sorted({r for v in EDGE_PAIRS.values() for r, _ in v}):
    RUNS["rows%d" % _rows] = Run("logistic", 3, edge_eps(_rows), N=_rows)
for _mass, _burn in MASS_ROWS:
    RUNS["mass_%s" % _mass] = Run("logistic", 3, edge_eps(40), mass=_mass, burn=_burn)
# which runs are made in float32 on the GPU (the CPU test runs the float32 oracle against the float64 oracle on exactly these)
F32_RUNS = sorted(["rows%d" % r for r, _ in EDGE_PAIRS[torch.float32]] + ["mass_%s" % m for m, _ in MASS_ROWS] + ["lds_logistic_1", "long"])


def deviation(a, b):
    """Largest difference per chain of two runs [n, C, D]."""
    return np.abs(a.astype(np.float64) - b.astype(np.float64)).max(axis=(0, 2))
