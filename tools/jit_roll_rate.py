#!/usr/bin/env python
"""Rate of sample() on a likelihood summed over data rows: the rolled callback kernel (hta_cb_rolled_kernel) at W = 1 and at the
host-chosen W - the latter with both forms of the table reads, direct and staged through LDS (HAMILTORCH_AMD_JIT_ROLL_TABLE) - against
the torch-evaluated route of the same library (native=False), in one process.

Workload: Bayesian logistic regression, D = 8, N = 2000 synthetic rows, L = 10, eps = 0.01, float32; 1024 and 65 536 chains.
Protocol: the module built and loaded (and the torch route warmed) before timing, 2 warm-up calls, then the median of 5 timed
sample() calls per route, each bracketed by device events around the whole call - table upload and the end-point check of the
compiled route included, since every caller pays them.  The routes are alternated.

    python tools/jit_roll_rate.py <tag> [out_dir]        ->  <out_dir or profiles>/<tag>_rolled.json
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HAMILTORCH_AMD_JIT_ROLL", "auto")      # the route under test is opt-in
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hamiltorch_amd as ht  # noqa: E402
from hamiltorch_amd import _abi, jit, samplers  # noqa: E402

WARMUP, TIMED = 2, 5
D, N, L, EPS = 8, 2000, 10, 0.01
TRAJ = {"rolled": 10, "generic": 3}
dev = torch.device("cuda:0")


def model():
    rng = np.random.default_rng(0)
    X = torch.tensor(rng.standard_normal((N, D)), dtype=torch.float32, device=dev)
    y = torch.tensor((rng.uniform(size=N) > 0.5).astype(np.float32), device=dev)
    return lambda w: (y * (X @ w) - torch.nn.functional.softplus(X @ w)).sum() - 0.5 * (w * w).sum()


def timed_call(fn, th0, route):
    samplers._CompiledRolledHMC.WAVES = 1 if route == "W=1" else None
    os.environ["HAMILTORCH_AMD_JIT_ROLL_TABLE"] = "lds" if route == "chosen-lds" else "direct"
    K = TRAJ["generic" if route == "generic" else "rolled"]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ht.sample(fn, th0, num_samples=K, num_steps_per_sample=L, step_size=EPS, verbose=False, seed=1, native=route != "generic")
    b.record()
    b.synchronize()
    r = _abi.last_route()
    assert ("hta_cb_rolled_kernel" in r) == (route != "generic"), r
    return th0.shape[0] * L * K / (a.elapsed_time(b) * 1e-3), r


def resources(comp):
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(comp.blob); f.flush()
        notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name], capture_output=True, text=True).stdout
    mine = next(b for b in re.split(r"\n\s+- \.agpr_count", notes) if re.search(r"\.name:\s+hta_cb_rolled_kernel\b", b))
    return {k: int(v) for k, v in re.findall(r"\.(vgpr_count|sgpr_count|vgpr_spill_count|private_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)", mine)}


def measure():
    fn = model()
    rows = []
    for C in (1024, 65536):
        th0 = (0.1 * torch.randn(C, D, generator=torch.Generator().manual_seed(2))).to(dev)
        routes = ("W=1", "chosen", "chosen-lds", "generic")
        rate, name = {r: [] for r in routes}, {}
        for r in routes:
            for _ in range(WARMUP):
                timed_call(fn, th0, r)
        for _ in range(TIMED):
            for r in routes:
                v, name[r] = timed_call(fn, th0, r)
                rate[r].append(v)
        med = {r: float(np.median(v)) for r, v in rate.items()}
        W = jit.runtime.rolled_waves(C, D, 0, N, 4)
        rows.append({"workload": "logistic", "D": D, "rows": N, "L": L, "eps": EPS, "chains": C, "dtype": "f32", "chosen_W": W,
                     "lds_bytes_per_workgroup": W * 64 * (1 + D) * 4, "chain_steps_per_s": {r: [float(x) for x in v] for r, v in rate.items()},
                     "median": med, "chosen_over_W1": med["chosen"] / med["W=1"], "chosen_over_generic": med["chosen"] / med["generic"],
                     "lds_over_direct": med["chosen-lds"] / med["chosen"],
                     "spread": max(float((max(v) - min(v)) / np.median(v)) for v in rate.values()), "routes": name})
        print(json.dumps(rows[-1]), flush=True)
    samplers._CompiledRolledHMC.WAVES = None
    os.environ["HAMILTORCH_AMD_JIT_ROLL_TABLE"] = jit.runtime.ROLLED_TABLE_DEFAULT
    comp = jit.compile_hmc(fn, th0[0], torch.float32, 0)
    return rows, resources(comp)


if __name__ == "__main__":
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
    rows, res = measure()
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "%s_rolled.json" % tag)
    with open(path, "w") as f:
        json.dump({"tool": "tools/jit_roll_rate.py", "device": torch.cuda.get_device_name(0), "warmup_calls": WARMUP, "timed_calls": TIMED,
                   "trajectories_per_call": TRAJ, "kernel": dict(res, name="hta_cb_rolled_kernel"),
                   "table_reads": {"chosen": "direct (wave-uniform loads through const T* __restrict__)",
                                   "chosen-lds": "a tile of rows per wave staged through LDS", "default": jit.runtime.ROLLED_TABLE_DEFAULT},
                   "rows": rows}, f, indent=1)
    print("wrote", path)
    sys.exit(0 if rows and all(r["chosen_over_generic"] > 1.0 for r in rows) else 1)
