"""Did the chains mix?  The 3-D correlated Gaussian of BASELINE config 2 (1024 chains, HMC, L = 25, eps = 0.3) sampled on the
MI355X engine, then bulk ESS and split R-hat of every coordinate computed where the samples are.

    python examples/diagnostics.py            (needs a GPU)
"""
import os
import sys
import time
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout
import hamiltorch_amd as hamiltorch  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    hamiltorch.set_random_seed(123)
    chains, draws = 1024, 1000
    cov = torch.tensor([[1.0, 0.6, 0.2], [0.6, 2.0, 0.5], [0.2, 0.5, 0.5]], device=dev)
    target = hamiltorch.GaussianTarget(torch.zeros(3, device=dev), covariance=cov)
    params_init = 0.1 * torch.randn(chains, 3, device=dev)
    out = hamiltorch.sample(target, params_init, num_samples=draws, num_steps_per_sample=25, step_size=0.3, verbose=False)
    torch.cuda.synchronize()
    t0 = time.time()
    s = hamiltorch.diagnostics.summary(out, skip=1)               # row 0 of the list is params_init
    dt = time.time() - t0
    print("%d draws x %d chains, diagnostics in %.2f ms" % (s.n_draws, s.n_chains, 1e3 * dt))
    print("  d      mean       sd   ess_bulk     rhat      tau  lags")
    for d in range(s.mean.numel()):
        print("%3d %9.4f %8.4f %10.1f %8.5f %8.3f %5d" % (d, float(s.mean[d]), float(s.sd[d]), float(s.ess_bulk[d]), float(s.rhat[d]),
                                                          float(s.tau[d]), int(s.lags_used[d])))
    print("min ESS %.1f, max R-hat %.5f (sd of the target: %s)" % (s.min_ess(), s.max_rhat(), [round(float(v) ** 0.5, 4) for v in cov.diag()]))


if __name__ == "__main__":
    main()
