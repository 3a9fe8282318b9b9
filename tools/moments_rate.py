#!/usr/bin/env python
"""Time of hamiltorch_amd.diagnostics.RunningMoments (update + result) against the same quantities composed from torch on the same
seeded device tensors, at the two shapes of tools/diag_rate.py - [1000, 1024, 3] and [200, 1024, 128], float32 -, fed in one
chunk and in 10 chunks; and the cross-chain warm-up (hamiltorch_amd.warmup) on the BASELINE config-2 target against the burn-in
of Sampler.HMC_NUTS of the same 450 trajectories.

    python tools/moments_rate.py <tag> <out_dir>      writes <out_dir>/<tag>_moments_rate.json

The torch composition: per chunk `x.double()`, `mean(0)` and the centred sum of squares, chunks merged by Chan's formula with
tensor arithmetic, then the pooled mean, within / between / total variance, R-hat and the regularised inverse mass from the
per-chain statistics.  Both paths: 2 warm-up calls, then alternated REPS times, each call between two device events, the second
one synchronised; medians and spread ((max - min) / median).  The two paths' results are compared (1e-9 relative).
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hamiltorch_amd as ht  # noqa: E402
from hamiltorch_amd import _abi  # noqa: E402
from hamiltorch_amd import diagnostics as DG  # noqa: E402

SHAPES = [(1000, 1024, 3), (200, 1024, 128)]
CHUNKS = (1, 10)
WARMUP, REPS = 2, 5
REG_N, REG_FLOOR = 5.0, 1e-3
SIGMA3 = [[1.0, 0.6, 0.2], [0.6, 2.0, 0.5], [0.2, 0.5, 0.5]]


def make(shape, dev):
    S, C, D = shape
    g = torch.Generator(device="cpu").manual_seed(S * 7 + D)
    x = torch.linspace(0.5, 3.0, D) * torch.randn(S, C, D, generator=g) + torch.linspace(-100.0, 100.0, D) + 0.3 * torch.randn(C, D, generator=g)
    return x.to(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def hand_written(x, k):
    acc = DG.RunningMoments()
    for part in x.chunk(k, dim=0):
        acc.update(part)
    r = acc.result(reg_n=REG_N, reg_floor=REG_FLOOR)
    return r.mean, r.var_within, r.var_between, r.var_total, r.rhat, r.inv_mass


def torch_composed(x, k):
    n, mean, m2 = 0.0, None, None
    for part in x.chunk(k, dim=0):
        xd = part.double()
        s = float(xd.shape[0])
        mb = xd.mean(0)
        qb = ((xd - mb) ** 2).sum(0)
        if mean is None:
            n, mean, m2 = s, mb, qb
        else:
            dl = mb - mean
            m2 = m2 + qb + dl * dl * (n * s / (n + s))
            mean = mean + dl * (s / (n + s))
            n += s
    C = float(x.shape[1])
    pooled = mean.mean(0)
    vw = (m2 / (n - 1.0)).mean(0)
    vb = mean.var(0, unbiased=True)
    N = n * C
    vt = (m2.sum(0) + n * ((mean - pooled) ** 2).sum(0)) / (N - 1.0)
    rhat = torch.sqrt(((n - 1.0) / n * vw + vb) / vw)
    im = (vt * (N / (N + REG_N)) + REG_FLOOR * (REG_N / (N + REG_N))).float()
    return pooled, vw, vb, vt, rhat, im


def rates(dev):
    rows = []
    for shape in SHAPES:
        x = make(shape, dev)
        for k in CHUNKS:
            new, old = (lambda: hand_written(x, k)), (lambda: torch_composed(x, k))
            for fn in (new, old):
                for _ in range(WARMUP):
                    timed(fn)
            secs = {"running_moments": [], "torch": []}
            for _ in range(REPS):
                dt, got = timed(new)
                secs["running_moments"].append(dt)
                dt, ref = timed(old)
                secs["torch"].append(dt)
            agree = max(float(((a.double() - b.double()).abs() / b.double().abs().clamp_min(1e-300)).max()) for a, b in zip(got[1:5], ref[1:5]))
            agree = max(agree, float((got[0] - ref[0]).abs().max() / x.abs().max()))
            med = {p: float(np.median(v)) for p, v in secs.items()}
            rows.append({"shape": list(shape), "dtype": "f32", "chunks": k, "seconds": secs, "median_seconds": med,
                         "spread": {p: float((max(v) - min(v)) / np.median(v)) for p, v in secs.items()},
                         "speedup": med["torch"] / med["running_moments"], "running_moments_is_slower": bool(med["running_moments"] > med["torch"]),
                         "segment_rows": DG.moments_segment_rows(-(-shape[0] // k), shape[1], shape[2]),
                         "relative_difference_to_torch": agree, "route": _abi.last_route()})
            assert agree <= 1e-9, rows[-1]
            print(json.dumps(rows[-1]), flush=True)
    return rows


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def warmup_against_nuts(dev):
    """cfg2's target (3-D correlated Gaussian, 1024 chains, L = 25) from eps0 = 0.3: warmup() of 450 trajectories against
    sample(sampler=HMC_NUTS, burn=450, num_samples=451), each twice (the first call pays the one-time set-up), wall-clock."""
    cov = torch.tensor(SIGMA3, dtype=torch.float32, device=dev)
    tgt = ht.GaussianTarget(torch.zeros(3, device=dev), covariance=cov)
    z = torch.empty(1024, 3, device=dev)
    _abi.momentum_resample(z, _abi.MASS_NONE, None, 0, 0, 0)
    start = (0.1 * z).contiguous()
    new = lambda: ht.warmup(tgt, start, num_steps_per_sample=25, step_size=0.3, seed=1)                              # noqa: E731
    old = lambda: ht.sample(tgt, start, num_samples=451, num_steps_per_sample=25, step_size=0.3, burn=450, sampler=ht.Sampler.HMC_NUTS,   # noqa: E731
                            debug=2, verbose=False, seed=1)
    secs = {"warmup": [], "hmc_nuts_burn": []}
    for _ in range(1 + REPS):
        dt, r = wall(new)
        secs["warmup"].append(dt)
        dt, (_, eps_nuts) = wall(old)
        secs["hmc_nuts_burn"].append(dt)
    first = {p: v[0] for p, v in secs.items()}
    secs = {p: v[1:] for p, v in secs.items()}
    med = {p: float(np.median(v)) for p, v in secs.items()}
    true_var = torch.tensor(SIGMA3).diagonal().double()
    out = {"target": "cfg2: 3-D correlated Gaussian, 1024 chains, L = 25, eps0 = 0.3", "trajectories": 450, "first_call_seconds": first, "seconds": secs,
           "median_seconds": med, "spread": {p: float((max(v) - min(v)) / np.median(v)) for p, v in secs.items()},
           "speedup": med["hmc_nuts_burn"] / med["warmup"], "warmup_step_size": r.step_size, "hmc_nuts_step_size": float(eps_nuts),
           "warmup_inv_mass_over_variance": (r.inv_mass.double().cpu() / true_var).tolist(), "host_reads": {"warmup": 45, "hmc_nuts_burn": 451}}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    tag, out_dir = sys.argv[1], sys.argv[2]
    os.makedirs(out_dir, exist_ok=True)
    dev = torch.device("cuda:0")
    res = {"tool": "tools/moments_rate.py", "device": torch.cuda.get_device_name(0), "warmup_calls": WARMUP, "alternated_calls": REPS,
           "rows": rates(dev), "warmup_against_hmc_nuts": warmup_against_nuts(dev)}
    path = os.path.join(out_dir, "%s_moments_rate.json" % tag)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)
