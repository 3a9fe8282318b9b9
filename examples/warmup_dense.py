#!/usr/bin/env python
"""Dense-mass warm-up (hamiltorch_amd.warmup(mass="dense")) against the diagonal one on a target whose badly scaled axes are not
the coordinate axes: a 6-D Gaussian with sd = (0.05, 0.2, 0.5, 1, 2, 5) along the columns of a random rotation, 64 chains, started
far from a sensible step size.  Both warm-ups run the default schedule (450 trajectories of L = 10); then 199 draws each.

The follow-up of the dense warm-up runs at L = 2: with a dense mass the target is close to a unit Gaussian in the mass's
coordinates, and a trajectory turns every coordinate by L * 2 asin(step_size / 2).  Near an even multiple of pi the chain returns
to where it started, near an odd one to its mirror image (the means look superbly mixed, the spread does not move) - the last line
prints that angle and the diagnostics of the same dense result at L = 10; judge it by the angle, not by its ESS.

    python examples/warmup_dense.py
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import hamiltorch_amd as ht  # noqa: E402

L, CHAINS, ROWS = 10, 64, 200


def follow_up(tgt, r, steps, seed):
    out, acc = ht.sample(tgt, r.params, num_samples=ROWS, num_steps_per_sample=steps, step_size=r.step_size, inv_mass=r.inv_mass, debug=2, verbose=False,
                         seed=seed)
    s = ht.diagnostics.summary(out, skip=1)
    turn = steps * 2.0 * math.asin(min(1.0, r.step_size / 2.0)) / math.pi
    return "L = %2d (turns by %.2f pi): max split R-hat %.3f, min bulk ESS %6.0f of %d draws, acceptance %.2f" % (
        steps, turn, s.max_rhat(), s.min_ess(), CHAINS * (ROWS - 1), float(acc.mean()))


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    Q = torch.linalg.qr(torch.randn(6, 6, generator=g, dtype=torch.float64))[0]
    sd = torch.tensor([0.05, 0.2, 0.5, 1.0, 2.0, 5.0], dtype=torch.float64)
    sigma = (Q * sd ** 2) @ Q.T
    tgt = ht.GaussianTarget(torch.zeros(6, device=dev), precision=((Q / sd ** 2) @ Q.T).float().to(dev))
    start = torch.randn(CHAINS, 6, generator=g).to(dev)
    diag = ht.warmup(tgt, start, num_steps_per_sample=L, step_size=0.01, seed=1)
    dense = ht.warmup(tgt, start, num_steps_per_sample=L, step_size=0.01, seed=1, mass="dense")
    F = torch.linalg.cholesky(torch.linalg.inv(dense.inv_mass.double().cpu()))
    eig = torch.linalg.eigvalsh(F.T @ sigma @ F)
    print("diagonal mass: step size %.4f" % diag.step_size)
    print("  " + follow_up(tgt, diag, L, 1000))
    print("dense mass   : step size %.4f, whitened eigenvalues %.3f .. %.3f (1 = the mass is the covariance)" % (dense.step_size, float(eig.min()), float(eig.max())))
    print("  " + follow_up(tgt, dense, 2, 1000))
    print("  " + follow_up(tgt, dense, L, 1000))


if __name__ == "__main__":
    main()
