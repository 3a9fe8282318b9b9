"""Shared by tests/test_adapt_dense_cpu.py and tests/test_gpu_adapt_dense.py: the two ROTATED targets of the dense warm-up tests,
the warm-up driven by the CPU oracle (oracle/hmc_oracle.py::sample_hmc on the engines' own Philox streams, the accumulator on the
numpy restatement of tests/cov_cases.py - tests/adapt_cases.py is the model), and the conditions both tests hold a run to.

Both runs: float32, 64 chains, L = 10 in the warm-up, the default schedule - blocks of 10 trajectories, windows of (5, 5, 10, 20)
blocks, 5 settle blocks: 450 trajectories -, then 199 draws (a sample() call of 200 rows).  The follow-up of the DENSE warm-up
runs at L = 2: with a dense mass the target is a unit Gaussian in the mass's coordinates and a trajectory turns every coordinate
by L * 2 asin(eps / 2); at the step sizes a dense warm-up ends at (0.7 to 1.2) and L = 10 that is close to 4 pi - the chain
returns to its start (R-hat 2.2, ESS 47 on the oracle with a correctly adapted mass).  The diagonal baseline keeps L = 10."""
from collections import namedtuple

import numpy as np

import adapt_cases as A
import cov_cases as CC
import hmc_oracle as O

L, L_DENSE, CHAINS, ROWS = A.L, 2, A.CHAINS, A.ROWS
FOLLOW_UP_SEED_INDEX = 45

Target = namedtuple("Target", "name scale rotation_seed eps0 seed start_seed")
GAUSS = Target("gauss", np.array([0.05, 0.2, 0.5, 1.0, 2.0, 5.0]), 5, 0.01, 4321, 0)
SECH = Target("sech", np.array([0.05, 0.3, 1.0, 4.0]), 5, 0.01, 77, 1)

#: the conditions (the oracle alone meets them on three rotations and several streams; measured ESS ratios: 70 x and up)
EIG_BAND = (0.8, 1.25)
ACCEPT_BAND = (0.65, 0.92)
RHAT_MAX = 1.05
ESS_RATIO = 10.0


def rotation(t):
    D = t.scale.size
    return np.linalg.qr(np.random.default_rng(t.rotation_seed).standard_normal((D, D)))[0]


def covariance(t):
    """The target's true covariance (float64): Q diag(v) Q^T, v = sd^2 (Gaussian) or (pi s / 2)^2 (hyperbolic secants)."""
    v = t.scale ** 2 if t.name == "gauss" else (np.pi * t.scale / 2.0) ** 2
    Q = rotation(t)
    return (Q * v) @ Q.T


def precision(t):
    Q = rotation(t)
    return (Q / t.scale ** 2) @ Q.T


def start(t, dtype=np.float32):
    return np.random.default_rng(t.start_seed).standard_normal((CHAINS, t.scale.size)).astype(dtype)


class RotatedSechTarget:
    """log p = -sum_k log cosh((Q^T theta)_k / s_k): a product of hyperbolic-secant densities along the columns of Q."""

    def __init__(self, s, Q):
        self.s, self.Q = np.asarray(s), np.asarray(Q)

    def logp(self, theta):
        z = np.abs((theta @ self.Q.astype(theta.dtype)) / self.s.astype(theta.dtype))
        return -np.sum(z + np.log1p(np.exp(-2 * z)) - theta.dtype.type(np.log(2.0)), axis=-1).astype(theta.dtype)

    def grad(self, theta):
        s, Q = self.s.astype(theta.dtype), self.Q.astype(theta.dtype)
        return -(np.tanh((theta @ Q) / s) / s) @ Q.T


def oracle_target(t, dtype=np.float32):
    if t.name == "gauss":
        return O.GaussianTarget(np.zeros(t.scale.size, dtype), precision(t).astype(dtype))
    return RotatedSechTarget(t.scale, rotation(t))


class NumpyCovariance:
    """The accumulator warmup_with() asks for under mass="dense", on the restatement of tests/cov_cases.py."""

    def __init__(self):
        self.state = CC.State()

    def update(self, rows, skip=0):
        self.state.update(np.stack([np.asarray(r) for r in rows])[skip:])
        return self

    def result(self, reg_n=None, reg_floor=1e-3, dtype=None):
        r = CC.finish(self.state.n, self.state.mean, self.state.q, 0.0 if reg_n is None else reg_n, reg_floor, slices=CC.SLICES)
        out = namedtuple("R", "inv_mass sd rhat n_draws")
        im = None if reg_n is None else r["inv_mass"].astype(np.float32 if dtype is None else dtype)
        return out(im, np.sqrt(np.diag(r["cov_total"])), r["rhat"], self.state.n)


def oracle_block(t, dtype=np.float32):
    """run_block of warmup_with() on the oracle: block k draws from PhiloxDraws(seed + k, arange(C))."""
    tgt = oracle_target(t, dtype)

    def run_block(params, n, eps, inv_mass, k):
        params = np.asarray(params, dtype=dtype)
        rows, info = O.sample_hmc(tgt, params, n, L, eps, 0, inv_mass, O.PhiloxDraws(t.seed + k, np.arange(params.shape[0]), dtype))
        return rows, info["acc_rate"]
    return run_block


def oracle_warmup(t, mass, dtype=np.float32):
    from hamiltorch_amd import adapt
    ctl = adapt.Controller(t.eps0, mass=mass)
    return adapt.warmup_with(oracle_block(t, dtype), start(t, dtype), ctl, NumpyCovariance if mass == "dense" else A.NumpyMoments)


def oracle_follow_up(t, r, steps, dtype=np.float32):
    """The ROWS-row run of `steps` leapfrog steps from a warm-up's result -> (draws[ROWS - 1, C, D], mean acceptance)."""
    rows, info = O.sample_hmc(oracle_target(t, dtype), np.asarray(r.params, dtype=dtype), ROWS, steps, r.step_size, 0, r.inv_mass,
                              O.PhiloxDraws(t.seed + FOLLOW_UP_SEED_INDEX, np.arange(CHAINS), dtype))
    return np.stack(rows)[1:], float(info["acc_rate"].mean())


def whitened_eigenvalues(t, inv_mass):
    """The eigenvalues of F^T Sigma F with Sigma the target's covariance and F F^T = inv_mass^-1 (float64): all 1 when the
    adapted inverse mass is exactly Sigma."""
    F = np.linalg.cholesky(np.linalg.inv(np.asarray(inv_mass, dtype=np.float64)))
    return np.linalg.eigvalsh(F.T @ covariance(t) @ F)


def check(name, windows, eig, acc, rhat, ess, ess_diag):
    """The conditions of a dense warm-up and its follow-up (printed first): all windows accepted, whitened eigenvalues, the
    follow-up's acceptance, split R-hat and min bulk ESS against the diagonal warm-up's follow-up."""
    print("%s: windows accepted %s | whitened eigenvalues %.3f..%.3f | follow-up at L = %d: acceptance %.4f rhat %.4f ess %.0f | diagonal "
          "warm-up's follow-up at L = %d: ess %.1f (ratio %.1f)" % (name, windows, eig.min(), eig.max(), L_DENSE, acc, rhat, ess, L, ess_diag, ess / ess_diag))
    assert len(windows) == 4 and all(windows), windows
    assert EIG_BAND[0] <= eig.min() and eig.max() <= EIG_BAND[1], eig
    assert ACCEPT_BAND[0] <= acc <= ACCEPT_BAND[1], acc
    assert rhat <= RHAT_MAX, rhat
    assert ess >= ESS_RATIO * ess_diag, (ess, ess_diag)
