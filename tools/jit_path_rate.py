#!/usr/bin/env python
"""Rate of samplers.leapfrog() on a (C, D) batch: the compiled path kernels (hta_cb_path_kernel / hta_cb_split_path_kernel) against
the torch-evaluated route of the same library (HAMILTORCH_AMD_JIT=0), in one process.

Workloads: the notebook funnel (D = 11), steps = 25, eps = 0.2, and a list of M = 3 logistic-regression subsets (D = 6) under
Integrator.SPLITTING, steps = 8, eps = 0.1; float32; 1024 and 65 536 chains.  Protocol: modules built (and the torch route's graphs
captured) before timing, 2 warm-up calls, then the median of 7 timed calls per route, each bracketed by device events around the whole
leapfrog() call - the end-point check of the compiled route included, since every caller pays it.  The routes are alternated.

    python tools/jit_path_rate.py <tag> [out_dir]        ->  <out_dir or profiles>/<tag>_path_leapfrog.json
Pass/fail: the compiled route is faster than the generic one in every row.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hamiltorch_amd as ht  # noqa: E402
from hamiltorch_amd import _abi  # noqa: E402

WARMUP, TIMED = 2, 7
HL2P = 0.9189385332046727
dev = torch.device("cuda:0")


def funnel(w):
    v, x = w[0], w[1:]
    return (-v * v / 18.0 - 1.0986122886681098 - HL2P) + (-0.5 * torch.exp(v) * (x * x).sum() + 0.5 * x.numel() * v - x.numel() * HL2P)


def logistic(M=3):
    rng = np.random.default_rng(0)
    X = rng.standard_normal((8 * M, 6)); y = (rng.uniform(size=8 * M) > 0.5).astype(np.float64)
    fns = []
    for m in range(M):
        A = torch.tensor(X[8 * m:8 * m + 8], dtype=torch.float32, device=dev)
        yy = torch.tensor(y[8 * m:8 * m + 8], dtype=torch.float32, device=dev)
        fns.append(lambda w, A=A, yy=yy: (yy * (A @ w) - torch.nn.functional.softplus(A @ w)).sum() - (0.5 / M) * (w * w).sum())
    return fns


WORKLOADS = [("funnel", funnel, 11, 25, 0.2, ht.Integrator.EXPLICIT, "hta_cb_path_kernel"),
             ("logistic-list-M3", None, 6, 8, 0.1, ht.Integrator.SPLITTING, "hta_cb_split_path_kernel")]


def timed_call(fn, th0, p0, steps, eps, integ, compiled, kernel):
    os.environ["HAMILTORCH_AMD_JIT"] = "1" if compiled else "0"
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = ht.samplers.leapfrog(th0, p0, fn, steps=steps, step_size=eps, sampler=ht.Sampler.HMC, integrator=integ)
    b.record()
    b.synchronize()
    r = _abi.last_route()
    assert (kernel in r) == compiled, r
    assert len(out[0]) == steps
    return a.elapsed_time(b) * 1e-3, r


def measure():
    rows = []
    for name, fn, D, steps, eps, integ, kernel in WORKLOADS:
        fn = logistic() if fn is None else fn
        for C in (1024, 65536):
            g = torch.Generator().manual_seed(2)
            th0 = (0.3 * torch.randn(C, D, generator=g)).to(dev)
            p0 = torch.randn(C, D, generator=g).to(dev)
            secs, route = {True: [], False: []}, {}
            for compiled in (True, False):
                for _ in range(WARMUP):
                    timed_call(fn, th0, p0, steps, eps, integ, compiled, kernel)
            for _ in range(TIMED):
                for compiled in (True, False):
                    dt, route[compiled] = timed_call(fn, th0, p0, steps, eps, integ, compiled, kernel)
                    secs[compiled].append(dt)
            rate = {k: C * steps / np.array(v) for k, v in secs.items()}
            med = {k: float(np.median(v)) for k, v in rate.items()}
            spread = max(float((v.max() - v.min()) / np.median(v)) for v in rate.values())
            rows.append({"workload": name, "D": D, "steps": steps, "eps": eps, "chains": C, "dtype": "f32",
                         "chain_steps_per_s": {"compiled": [float(x) for x in rate[True]], "generic": [float(x) for x in rate[False]]},
                         "median": {"compiled": med[True], "generic": med[False]}, "ratio": med[True] / med[False], "spread": spread,
                         "compiled_is_faster": bool(med[True] > med[False]), "route": route[True], "generic_route": route[False]})
            print(json.dumps(rows[-1]), flush=True)
    return rows


if __name__ == "__main__":
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
    rows = measure()
    os.environ.pop("HAMILTORCH_AMD_JIT", None)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "%s_path_leapfrog.json" % tag)
    with open(path, "w") as f:
        json.dump({"tool": "tools/jit_path_rate.py", "device": torch.cuda.get_device_name(0), "warmup_calls": WARMUP, "timed_calls": TIMED,
                   "rows": rows}, f, indent=1)
    print("wrote", path)
    sys.exit(0 if rows and all(r["compiled_is_faster"] for r in rows) else 1)
