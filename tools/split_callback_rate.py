#!/usr/bin/env python
"""Rate of the compiled split-HMC route (hta_cb_split_kernel) against the torch-evaluated generic route of the same library
(HAMILTORCH_AMD_JIT=0), through sample() with a device synchronise, one process, the two routes alternated three times.

Instances: Bayesian logistic regression (D = 6, 24 rows, M = 3 plain closures: tests/test_gpu_jit_split.py) and a 1-5-5-1 tanh MLP
(D = 46, M = 3, plain closures) when it compiles within the operation limit; 1024 and 65 536 chains, L = 8, Integrator.SPLITTING,
float32.  Trajectory counts are calibrated per route so that a timed call lasts at least a second after a warm-up call.

    python tools/split_callback_rate.py <tag>        ->  profiles/<tag>_split_callback.json
Pass/fail: at 1024 chains the compiled route must beat the generic one by more than the measured spread.
"""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hamiltorch_amd as ht  # noqa: E402
from hamiltorch_amd import _abi, jit  # noqa: E402

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
L, M = 8, 3
dev = torch.device("cuda:0")


def logistic():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((24, 6)); y = (rng.uniform(size=24) > 0.5).astype(np.float64)
    fns = []
    for m in range(M):
        A = torch.tensor(X[8 * m:8 * m + 8], dtype=torch.float32, device=dev)
        yy = torch.tensor(y[8 * m:8 * m + 8], dtype=torch.float32, device=dev)
        fns.append(lambda w, A=A, yy=yy: (yy * (A @ w) - torch.nn.functional.softplus(A @ w)).sum() - (0.5 / M) * (w * w).sum())
    return fns, 6, 0.1


def mlp():
    g = torch.Generator().manual_seed(0)
    X = torch.randn(24, 1, generator=g).to(dev); Y = torch.sin(3 * X) + 0.1 * torch.randn(24, 1, generator=g).to(dev)
    fns = []
    for m in range(M):
        x, y = X[8 * m:8 * m + 8], Y[8 * m:8 * m + 8]

        def f(w, x=x, y=y):
            h = torch.tanh(x @ w[0:5].reshape(1, 5) + w[5:10])
            h = torch.tanh(h @ w[10:35].reshape(5, 5) + w[35:40])
            out = h @ w[40:45].reshape(5, 1) + w[45]
            return -0.5 * 4.0 * ((out - y) ** 2).sum() - (0.5 / M) * (w * w).sum()
        fns.append(f)
    return fns, 46, 0.01


def resources(comp):
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(comp.blob); f.flush()
        notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True).stdout
    return {k: int(v) for k, v in re.findall(r"\.(vgpr_count|sgpr_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", notes)}


def call(fns, th0, eps, N, compiled):
    os.environ["HAMILTORCH_AMD_JIT"] = "1" if compiled else "0"
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    ht.sample(fns, th0, num_samples=N, num_steps_per_sample=L, step_size=eps, burn=N - 2, integrator=ht.Integrator.SPLITTING,
              verbose=False, seed=1)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    r = _abi.last_route()
    assert ("hta_cb_split_kernel" in r) == compiled, r
    return dt, r


def calibrate(fns, th0, eps, compiled):
    N = 8
    call(fns, th0, eps, N, compiled)                        # warm-up: trace, hipRTC, module load / vmap and graph capture
    while True:
        dt, _ = call(fns, th0, eps, N, compiled)
        if dt >= 1.0 or N >= (1 << 22):
            return N
        N = int(min(1 << 22, max(2 * N, N * 1.3 / max(dt, 1e-4))))


def measure(name, make):
    fns, D, eps = make()
    rows = []
    try:
        comp = jit.compile_split(fns, torch.zeros(D, device=dev), torch.float32, 0)
    except jit.Unsupported as e:
        return [{"instance": name, "D": D, "M": M, "compiled": False, "reason": str(e)}]
    res = resources(comp)
    for C in (1024, 65536):
        th0 = 0.3 * torch.randn(C, D, generator=torch.Generator().manual_seed(2)).to(dev)
        n = {True: calibrate(fns, th0, eps, True), False: calibrate(fns, th0, eps, False)}
        rates = {True: [], False: []}
        route = {}
        for _ in range(3):
            for compiled in (True, False):
                dt, route[compiled] = call(fns, th0, eps, n[compiled], compiled)
                rates[compiled].append(C * n[compiled] * L / dt)
        a, b = np.array(rates[True]), np.array(rates[False])
        spread = max((a.max() - a.min()) / np.median(a), (b.max() - b.min()) / np.median(b))
        ratio = float(np.median(a) / np.median(b))
        rows.append({"instance": name, "D": D, "M": M, "L": L, "chains": C, "dtype": "f32", "compiled": True,
                     "trajectories": {"compiled": n[True], "generic": n[False]},
                     "chain_steps_per_s": {"compiled": [float(x) for x in a], "generic": [float(x) for x in b]},
                     "median": {"compiled": float(np.median(a)), "generic": float(np.median(b))}, "spread": float(spread), "ratio": ratio,
                     "compiled_is_faster_beyond_spread": bool(np.median(a) > np.median(b) * (1.0 + spread)),
                     "route": route[True], "generic_route": route[False], "code_object": res})
        print(json.dumps(rows[-1]), flush=True)
    return rows


if __name__ == "__main__":
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
    rows = measure("logistic", logistic) + measure("mlp-1-5-5-1", mlp)
    os.environ.pop("HAMILTORCH_AMD_JIT", None)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "%s_split_callback.json" % tag)
    with open(path, "w") as f:
        json.dump({"tool": "tools/split_callback_rate.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    print("wrote", path)
    at_1024 = [r for r in rows if r.get("chains") == 1024]
    sys.exit(0 if at_1024 and all(r["compiled_is_faster_beyond_spread"] for r in at_1024) else 1)
