"""Shared by tests/test_adapt_cpu.py and tests/test_gpu_adapt.py: the two targets of the warm-up tests, the warm-up driven by the
CPU oracle (oracle/hmc_oracle.py::sample_hmc on the engines' own Philox streams, the moments from the numpy restatement of
tests/moments_cases.py), the HMC_NUTS baseline of the same budget, and the diagnostics of a run in numpy.

Both runs: 64 chains, L = 10, the default schedule - blocks of 10 trajectories, windows of (5, 5, 10, 20) blocks, 5 settle
blocks: 450 trajectories -, then 199 draws (a sample() call of 200 rows)."""
from collections import namedtuple

import numpy as np

import hmc_oracle as O
import moments_cases as MC

L, CHAINS, ROWS, BURN = 10, 64, 200, 450

Target = namedtuple("Target", "name scale eps0 seed start_seed variance")
GAUSS = Target("gauss", np.array([0.05, 0.5, 1.0, 5.0]), 0.01, 1234, 0, np.array([0.05, 0.5, 1.0, 5.0]) ** 2)
SECH = Target("sech", np.array([0.2, 1.0, 5.0]), 0.02, 77, 1, (np.pi * np.array([0.2, 1.0, 5.0]) / 2.0) ** 2)


def start(t, dtype=np.float32):
    return np.random.default_rng(t.start_seed).standard_normal((CHAINS, t.scale.size)).astype(dtype)


class SechTarget:
    """log p = -sum log cosh(theta / s): a product of hyperbolic-secant densities, variance (pi s / 2)^2 per coordinate."""

    def __init__(self, s):
        self.s = np.asarray(s)

    def logp(self, theta):
        z = np.abs(theta / self.s.astype(theta.dtype))
        return -np.sum(z + np.log1p(np.exp(-2 * z)) - theta.dtype.type(np.log(2.0)), axis=-1).astype(theta.dtype)

    def grad(self, theta):
        s = self.s.astype(theta.dtype)
        return -np.tanh(theta / s) / s


def oracle_target(t, dtype=np.float32):
    if t.name == "gauss":
        return O.GaussianTarget(np.zeros(t.scale.size, dtype), np.diag(1.0 / t.scale ** 2).astype(dtype))
    return SechTarget(t.scale)


class NumpyMoments:
    """The accumulator warmup_with() asks for, on the restatement of tests/moments_cases.py."""

    def __init__(self):
        self.state = MC.State()

    def update(self, rows, skip=0):
        self.state.update(np.stack([np.asarray(r) for r in rows])[skip:])
        return self

    def result(self, reg_n=None, reg_floor=1e-3, dtype=None):
        r = MC.finish(self.state.n, self.state.mean, self.state.m2, 0.0 if reg_n is None else reg_n, reg_floor, slices=MC.SLICES)
        out = namedtuple("R", "inv_mass sd rhat n_draws")
        im = None if reg_n is None else r["inv_mass"].astype(np.float32 if dtype is None else dtype)
        return out(im, np.sqrt(r["var_total"]), r["rhat"], self.state.n)


def oracle_block(t, dtype=np.float32):
    """run_block of warmup_with() on the oracle: block k draws from PhiloxDraws(seed + k, arange(C))."""
    tgt = oracle_target(t, dtype)

    def run_block(params, n, eps, inv_mass, k):
        params = np.asarray(params, dtype=dtype)
        rows, info = O.sample_hmc(tgt, params, n, L, eps, 0, inv_mass, O.PhiloxDraws(t.seed + k, np.arange(params.shape[0]), dtype))
        return rows, info["acc_rate"]
    return run_block


def oracle_warmup(t, dtype=np.float32, **controller_args):
    from hamiltorch_amd import adapt
    ctl = adapt.Controller(t.eps0, **controller_args)
    return adapt.warmup_with(oracle_block(t, dtype), start(t, dtype), ctl, NumpyMoments), ctl


def oracle_follow_up(t, r, seed_index, dtype=np.float32):
    """The ROWS-row run from a warm-up's result -> (draws[ROWS - 1, C, D], mean acceptance)."""
    rows, info = O.sample_hmc(oracle_target(t, dtype), np.asarray(r.params, dtype=dtype), ROWS, L, r.step_size, 0, r.inv_mass,
                              O.PhiloxDraws(t.seed + seed_index, np.arange(CHAINS), dtype))
    return np.stack(rows)[1:], float(info["acc_rate"].mean())


def oracle_nuts(t, dtype=np.float32):
    """The same budget as Sampler.HMC_NUTS: burn = 450, 650 trajectories, identity mass, the same start -> (draws, step size)."""
    rows, info = O.sample_hmc(oracle_target(t, dtype), start(t, dtype), BURN + ROWS, L, t.eps0, BURN, None,
                              O.PhiloxDraws(t.seed, np.arange(CHAINS), dtype), nuts_desired=0.8)
    return np.stack(rows)[1:], info["step_size"]


def diagnostics(x):
    """x[S, C, D] -> (max split R-hat, min bulk ESS) with the definitions of hamiltorch_amd/ess.py."""
    import torch
    from hamiltorch_amd import ess as E
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return E.rhat_max(xt), E.ess_min(xt)
