"""Did the chains mix?  The 3-D correlated Gaussian of BASELINE config 2 (1024 chains, HMC, L = 25, eps = 0.3) and the funnel of
examples/funnel.py (256 chains, HMC) sampled on the MI355X engine, then the diagnostics of every coordinate computed where the samples
are: summary() (moment-based bulk ESS and split R-hat) next to rank_summary() (rank-normalised bulk and tail ESS, rank-normalised and
folded R-hat, the quantiles - what Stan and ArviZ print).  On the Gaussian the two should agree; the funnel's x coordinates are
heavy-tailed with a scale that depends on v, which is where the folded R-hat (chains that differ in scale) and the tail ESS (how many
effective draws the 5 % / 95 % quantiles rest on) say more than the moment-based statistics.

    python examples/diagnostics.py            (needs a GPU)
"""
import os
import sys
import time
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a checkout
import hamiltorch_amd as hamiltorch  # noqa: E402
from examples.funnel import D as FUNNEL_D, funnel_ll  # noqa: E402


def report(name, out, skip):
    torch.cuda.synchronize()
    t0 = time.time()
    s = hamiltorch.diagnostics.summary(out, skip=skip)            # row 0 of the list is params_init
    t1 = time.time()
    r = hamiltorch.diagnostics.rank_summary(out, skip=skip)
    t2 = time.time()
    print("%s: %d draws x %d chains, summary() in %.2f ms, rank_summary() in %.2f ms" % (name, s.n_draws, s.n_chains, 1e3 * (t1 - t0), 1e3 * (t2 - t1)))
    print("        summary()                                | rank_summary()")
    print("  d      mean       sd   ess_bulk     rhat  lags |   ess_bulk   ess_tail     rhat   folded       q05    median       q95")
    for d in range(s.mean.numel()):
        print("%3d %9.4f %8.4f %10.1f %8.5f %5d | %10.1f %10.1f %8.5f %8.5f %9.4f %9.4f %9.4f"
              % (d, float(s.mean[d]), float(s.sd[d]), float(s.ess_bulk[d]), float(s.rhat[d]), int(s.lags_used[d]), float(r.ess_bulk[d]), float(r.ess_tail[d]),
                 float(r.rhat[d]), float(r.rhat_folded[d]), float(r.q05[d]), float(r.median[d]), float(r.q95[d])))
    print("summary(): min ESS %.1f, max R-hat %.5f | rank_summary(): min ESS (bulk, tail) %.1f, max R-hat %.5f\n" % (s.min_ess(), s.max_rhat(), r.min_ess(), r.max_rhat()))


def main():
    dev = torch.device("cuda:0")
    hamiltorch.set_random_seed(123)
    chains, draws = 1024, 1000
    cov = torch.tensor([[1.0, 0.6, 0.2], [0.6, 2.0, 0.5], [0.2, 0.5, 0.5]], device=dev)
    target = hamiltorch.GaussianTarget(torch.zeros(3, device=dev), covariance=cov)
    params_init = 0.1 * torch.randn(chains, 3, device=dev)
    out = hamiltorch.sample(target, params_init, num_samples=draws, num_steps_per_sample=25, step_size=0.3, verbose=False)
    report("Gaussian (sd of the target: %s)" % [round(float(v) ** 0.5, 4) for v in cov.diag()], out, 1)

    params_init = torch.ones(256, FUNNEL_D, device=dev)
    params_init[:, 0] = 0.0
    out = hamiltorch.sample(log_prob_func=funnel_ll, params_init=params_init, num_samples=400, step_size=0.2, num_steps_per_sample=25, verbose=False)
    report("funnel (v = coordinate 0 ~ N(0, 3^2), x ~ N(0, exp(-v)))", out, len(out) // 2)


if __name__ == "__main__":
    main()
