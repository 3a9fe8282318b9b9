#!/usr/bin/env python
"""Bayesian logistic regression on a data set of a few thousand rows: an ordinary closure over the data, sampled with plain HMC.

The callable is traced, ROLLED over its rows (one term function + a table of per-row constants, hamiltorch_amd/jit/roll.py) and
compiled into the rolled trajectory kernel; `hta_last_route()` names the kernel.  The route is opt-in (HAMILTORCH_AMD_JIT_ROLL=auto,
set below); without it the same call runs on the torch-evaluated route.  The data are synthetic, generated here.

    python examples/logistic_regression.py [rows] [chains]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HAMILTORCH_AMD_JIT_ROLL", "auto")
import torch  # noqa: E402

import hamiltorch_amd as ht  # noqa: E402
from hamiltorch_amd import _abi  # noqa: E402


def main(rows=2000, chains=1024, D=8):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    w_true = torch.randn(D, generator=g)
    X = torch.randn(rows, D, generator=g)
    y = (torch.rand(rows, generator=g) < torch.sigmoid(X @ w_true)).float()
    X, y = X.to(dev), y.to(dev)

    def log_prob(w):
        z = X @ w
        return (y * z - torch.nn.functional.softplus(z)).sum() - 0.5 * (w * w).sum()

    theta0 = 0.1 * torch.randn(chains, D, generator=g).to(dev)
    samples, acc = ht.sample(log_prob, theta0, num_samples=300, num_steps_per_sample=10, step_size=0.02, burn=100, debug=2, verbose=False)
    print("route:", _abi.last_route())
    post = torch.stack(list(samples))[1:].mean(dim=(0, 1)).cpu()
    print("acceptance %.2f" % float(acc.mean()))
    print("posterior mean:", [round(float(v), 2) for v in post])
    print("generating w:  ", [round(float(v), 2) for v in w_true])


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
