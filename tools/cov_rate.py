#!/usr/bin/env python
"""Time of hamiltorch_amd.diagnostics.RunningCovariance (update + result) against the same quantities composed from torch on the
same seeded device tensors, at [1000, 1024, 3] and [200, 1024, 64], float32, fed in one chunk and in 10 chunks; and the dense
cross-chain warm-up (hamiltorch_amd.warmup(mass="dense")) on the BASELINE config-2 target against the diagonal one.

    python tools/cov_rate.py <tag> <out_dir>      writes <out_dir>/<tag>_cov_rate.json

The torch composition: per chunk `x.double()`, `mean(0)` and the centred co-moments by one `einsum("scd,sce->cde")`, chunks merged
by Chan's formula with tensor arithmetic, then the pooled mean, the within and total covariance, R-hat and the regularised inverse
mass from the per-chain statistics.  Both paths: 2 warm-up calls, then alternated REPS times, each call between two device
events, the second one synchronised; medians and spread ((max - min) / median).  The two paths' results are compared (1e-9 of
the largest entry).  No speed-up is claimed here: `running_covariance_is_slower` says where the hand-written path loses.
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

SHAPES = [(1000, 1024, 3), (200, 1024, 64)]
CHUNKS = (1, 10)
WARMUP, REPS = 2, 5
REG_N, REG_FLOOR = 5.0, 1e-3
SIGMA3 = [[1.0, 0.6, 0.2], [0.6, 2.0, 0.5], [0.2, 0.5, 0.5]]


def make(shape, dev):
    S, C, D = shape
    g = torch.Generator(device="cpu").manual_seed(S * 7 + D)
    mix = torch.eye(D) + 0.5 * torch.randn(D, D, generator=g) / D ** 0.5
    x = (torch.linspace(0.5, 3.0, D) * torch.randn(S, C, D, generator=g)) @ mix + torch.linspace(-100.0, 100.0, D) + 0.3 * torch.randn(C, D, generator=g)
    return x.to(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def hand_written(x, k):
    acc = DG.RunningCovariance()
    for part in x.chunk(k, dim=0):
        acc.update(part)
    r = acc.result(reg_n=REG_N, reg_floor=REG_FLOOR)
    return r.mean, r.cov_within, r.cov_total, r.rhat, r.inv_mass


def torch_composed(x, k):
    n, mean, q = 0.0, None, None
    for part in x.chunk(k, dim=0):
        xd = part.double()
        s = float(xd.shape[0])
        mb = xd.mean(0)
        d = xd - mb
        qb = torch.einsum("scd,sce->cde", d, d)
        if mean is None:
            n, mean, q = s, mb, qb
        else:
            dl = mb - mean
            q = q + qb + dl[:, :, None] * dl[:, None, :] * (n * s / (n + s))
            mean = mean + dl * (s / (n + s))
            n += s
    C = float(x.shape[1])
    pooled = mean.mean(0)
    cw = (q / (n - 1.0)).mean(0)
    N = n * C
    dm = mean - pooled
    ct = (q.sum(0) + n * (dm.T @ dm)) / (N - 1.0)
    vw, vb = cw.diagonal(), mean.var(0, unbiased=True)
    rhat = torch.sqrt(((n - 1.0) / n * vw + vb) / vw)
    im = (ct * (N / (N + REG_N)) + REG_FLOOR * (REG_N / (N + REG_N)) * torch.eye(x.shape[2], dtype=ct.dtype, device=ct.device)).float()
    return pooled, cw, ct, rhat, im


def rates(dev):
    rows = []
    for shape in SHAPES:
        x = make(shape, dev)
        for k in CHUNKS:
            new, old = (lambda: hand_written(x, k)), (lambda: torch_composed(x, k))
            for fn in (new, old):
                for _ in range(WARMUP):
                    timed(fn)
            secs = {"running_covariance": [], "torch": []}
            for _ in range(REPS):
                dt, got = timed(new)
                secs["running_covariance"].append(dt)
                dt, ref = timed(old)
                secs["torch"].append(dt)
            agree = max(float((a.double() - b.double()).abs().max() / b.double().abs().max()) for a, b in zip(got[1:], ref[1:]))
            agree = max(agree, float((got[0] - ref[0]).abs().max() / x.abs().max()))
            med = {p: float(np.median(v)) for p, v in secs.items()}
            rows.append({"shape": list(shape), "dtype": "f32", "chunks": k, "seconds": secs, "median_seconds": med,
                         "spread": {p: float((max(v) - min(v)) / np.median(v)) for p, v in secs.items()},
                         "speedup": med["torch"] / med["running_covariance"], "running_covariance_is_slower": bool(med["running_covariance"] > med["torch"]),
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


def dense_against_diagonal(dev):
    """cfg2's target (3-D correlated Gaussian, 1024 chains, L = 25) from eps0 = 0.3: warmup(mass="dense") against warmup() of
    the same 450 trajectories, each once for the one-time set-up and then REPS times alternated, wall-clock."""
    cov = torch.tensor(SIGMA3, dtype=torch.float32, device=dev)
    tgt = ht.GaussianTarget(torch.zeros(3, device=dev), covariance=cov)
    z = torch.empty(1024, 3, device=dev)
    _abi.momentum_resample(z, _abi.MASS_NONE, None, 0, 0, 0)
    start = (0.1 * z).contiguous()
    new = lambda: ht.warmup(tgt, start, num_steps_per_sample=25, step_size=0.3, seed=1, mass="dense")      # noqa: E731
    old = lambda: ht.warmup(tgt, start, num_steps_per_sample=25, step_size=0.3, seed=1)                    # noqa: E731
    secs = {"dense": [], "diagonal": []}
    for _ in range(1 + REPS):
        dt, r = wall(new)
        secs["dense"].append(dt)
        route = _abi.last_route()
        dt, rd = wall(old)
        secs["diagonal"].append(dt)
    first = {p: v[0] for p, v in secs.items()}
    secs = {p: v[1:] for p, v in secs.items()}
    med = {p: float(np.median(v)) for p, v in secs.items()}
    true = torch.tensor(SIGMA3).double()
    F = torch.linalg.cholesky(torch.linalg.inv(r.inv_mass.double().cpu()))
    out = {"target": "cfg2: 3-D correlated Gaussian, 1024 chains, L = 25, eps0 = 0.3", "trajectories": 450, "first_call_seconds": first, "seconds": secs,
           "median_seconds": med, "spread": {p: float((max(v) - min(v)) / np.median(v)) for p, v in secs.items()},
           "dense_over_diagonal": med["dense"] / med["diagonal"], "dense_step_size": r.step_size, "diagonal_step_size": rd.step_size,
           "dense_whitened_eigenvalues": torch.linalg.eigvalsh(F.T @ true @ F).tolist(),
           "diagonal_inv_mass_over_variance": (rd.inv_mass.double().cpu() / true.diagonal()).tolist(), "dense_route": route}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    tag, out_dir = sys.argv[1], sys.argv[2]
    os.makedirs(out_dir, exist_ok=True)
    dev = torch.device("cuda:0")
    res = {"tool": "tools/cov_rate.py", "device": torch.cuda.get_device_name(0), "warmup_calls": WARMUP, "alternated_calls": REPS,
           "rows": rates(dev), "dense_warmup_against_diagonal": dense_against_diagonal(dev)}
    path = os.path.join(out_dir, "%s_cov_rate.json" % tag)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)
