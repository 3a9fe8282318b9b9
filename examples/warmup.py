#!/usr/bin/env python
"""Cross-chain warm-up (hamiltorch_amd.warmup): a step size and a diagonal mass for a batch of chains, then the run they are for.

Two targets, 64 chains each, L = 10, started far from a sensible step size:
  * an anisotropic Gaussian, sd = (0.05, 0.5, 1, 5), on the Gaussian kernels;
  * a closure the library has never seen, log p = -sum log cosh(theta / s) with s = (0.2, 1, 5), compiled into the trajectory kernel.
For each: `diagnostics.summary` of 199 draws after Sampler.HMC_NUTS with the same budget (burn = 450, identity mass) and after
warmup() (450 trajectories: 45 blocks of 10, the acceptance rate read once per block, the mass pooled over chains per window).

    python examples/warmup.py
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import hamiltorch_amd as ht  # noqa: E402
from hamiltorch_amd import _abi  # noqa: E402

L, CHAINS, ROWS, BURN = 10, 64, 200, 450


def compare(name, log_prob, start, eps0, variance, seed):
    print("== %s, step size %g to start from ==" % (name, eps0))
    out = ht.sample(log_prob, start, num_samples=BURN + ROWS, num_steps_per_sample=L, step_size=eps0, burn=BURN, sampler=ht.Sampler.HMC_NUTS,
                    verbose=False, seed=seed)
    before = ht.diagnostics.summary(out, skip=1)
    print("HMC_NUTS burn-in, identity mass : max split R-hat %.3f, min bulk ESS %.0f of %d draws" % (before.max_rhat(), before.min_ess(), CHAINS * (ROWS - 1)))
    r = ht.warmup(log_prob, start, num_steps_per_sample=L, step_size=eps0, seed=seed)
    route = _abi.last_route()
    out, acc = ht.sample(log_prob, r.params, num_samples=ROWS, num_steps_per_sample=L, step_size=r.step_size, inv_mass=r.inv_mass, debug=2,
                         verbose=False, seed=seed + 1000)
    after = ht.diagnostics.summary(out, skip=1)
    print("warmup()                        : max split R-hat %.3f, min bulk ESS %.0f, acceptance %.2f" % (after.max_rhat(), after.min_ess(), float(acc.mean())))
    print("  step size %.4f, inv_mass / variance %s, blocks on %s" % (r.step_size, [round(v, 3) for v in (r.inv_mass.double().cpu() / variance).tolist()], route))
    for h in r.history:
        if h["kind"] == "window":
            print("  window of phase %d: %d draws per chain, max R-hat %.3f" % (h["phase"], h["n_draws"], float(h["rhat"].max())))


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    sd = torch.tensor([0.05, 0.5, 1.0, 5.0], device=dev)
    gauss = ht.GaussianTarget(torch.zeros(4, device=dev), precision=torch.diag(1.0 / (sd * sd)))
    compare("anisotropic Gaussian", gauss, torch.randn(CHAINS, 4).to(dev), 0.01, (sd * sd).double().cpu(), 1234)
    s = torch.tensor([0.2, 1.0, 5.0], device=dev)
    sech = lambda th: -torch.log(torch.cosh(th / s)).sum()                   # noqa: E731
    compare("product of sech densities (compiled closure)", sech, torch.randn(CHAINS, 3).to(dev), 0.02, ((math.pi * s / 2) ** 2).double().cpu(), 77)


if __name__ == "__main__":
    main()
