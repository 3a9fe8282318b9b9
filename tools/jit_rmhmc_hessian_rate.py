#!/usr/bin/env python
"""Rate of sample(sampler=RMHMC, integrator=EXPLICIT, metric=HESSIAN) on a general callable: the compiled trajectory kernel
(hta_cb_rmhmc_hess_kernel) against the launch-per-evaluation route of the same library (HAMILTORCH_AMD_JIT=0: torch.func derivatives
+ one hta_metric_eval launch per evaluation), in one process - and the register / scratch counts of the kernel.

Workload: the log-cosh target (oracle.LogCoshTarget's form) at D = 8, float32, L = 10, eps = 0.1, jitter 1e-3, TRAJ trajectories per
call; 1024 and 65 536 chains.  Protocol: modules built (and the torch route's functions traced) before timing, 2 warm-up calls, then the
median of 7 timed calls per route, each bracketed by device events around the whole sample() call - the end-of-run check of the
compiled route included, since every caller pays it.  The routes are alternated.  No rate is asked for: the number is the ratio.

    python tools/jit_rmhmc_hessian_rate.py [rates] [out_dir]      (needs the GPU)   "rows" of <out_dir or profiles>/r12a_rmhmc_hessian.json
    python tools/jit_rmhmc_hessian_rate.py resources [out_dir]    (hipRTC only)     "resources" of the same file: the counts of
        tests/test_jit_rmhmc_hessian_cpu.py::test_symbols_and_resources, next to the soft-abs kernel's for the same callable
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

WARMUP, TIMED = 2, 7
D, L, EPS, JITTER, TRAJ = 8, 10, 0.1, 1e-3, 5
KERNEL = "hta_cb_rmhmc_hess_kernel"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
NAME = "r12a_rmhmc_hessian.json"


def logcosh(D, device=None):
    """-1/2 w^T P w - sum log cosh(A w), P = Q diag(linspace(0.5, 2, D)) Q^T, A = 0.6 randn(D + 2, D) (default_rng(2): Q, then A)."""
    rng = np.random.default_rng(2)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    P = (Q * np.linspace(0.5, 2.0, D)) @ Q.T
    P = 0.5 * (P + P.T)
    A = 0.6 * rng.standard_normal((D + 2, D))

    def f(w):
        Pt = torch.as_tensor(P, dtype=w.dtype, device=w.device); At = torch.as_tensor(A, dtype=w.dtype, device=w.device)
        return -0.5 * torch.dot(w, torch.mv(Pt, w)) - torch.log(torch.cosh(torch.mv(At, w))).sum()
    return f


def timed_call(ht, fn, th0, compiled):
    from hamiltorch_amd import _abi
    os.environ["HAMILTORCH_AMD_JIT"] = "1" if compiled else "0"
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = ht.sample(fn, th0, num_samples=TRAJ, num_steps_per_sample=L, step_size=EPS, jitter=JITTER, explicit_binding_const=10.0,
                    sampler=ht.Sampler.RMHMC, integrator=ht.Integrator.EXPLICIT, metric=ht.Metric.HESSIAN, verbose=False, seed=3)
    b.record()
    b.synchronize()
    r = _abi.last_route()
    assert (KERNEL in r) == compiled, r
    assert len(out) == TRAJ
    return a.elapsed_time(b) * 1e-3, r


def rates():
    import hamiltorch_amd as ht
    dev = torch.device("cuda:0")
    fn = logcosh(D)
    rows = []
    for C in (1024, 65536):
        g = torch.Generator().manual_seed(2)
        th0 = (0.4 * torch.randn(C, D, generator=g)).to(dev)
        secs, route = {True: [], False: []}, {}
        for compiled in (True, False):
            for _ in range(WARMUP):
                timed_call(ht, fn, th0, compiled)
        for _ in range(TIMED):
            for compiled in (True, False):
                dt, route[compiled] = timed_call(ht, fn, th0, compiled)
                secs[compiled].append(dt)
        rate = {k: C * TRAJ * L / np.array(v) for k, v in secs.items()}
        med = {k: float(np.median(v)) for k, v in rate.items()}
        spread = {k: float((v.max() - v.min()) / np.median(v)) for k, v in rate.items()}
        rows.append({"workload": "logcosh", "D": D, "L": L, "eps": EPS, "jitter": JITTER, "trajectories_per_call": TRAJ, "chains": C, "dtype": "f32",
                     "chain_steps_per_s": {"compiled": [float(x) for x in rate[True]], "launch_sequence": [float(x) for x in rate[False]]},
                     "median": {"compiled": med[True], "launch_sequence": med[False]}, "ratio": med[True] / med[False],
                     "spread": {"compiled": spread[True], "launch_sequence": spread[False]},
                     "compiled_is_faster": bool(med[True] > med[False]), "route": route[True], "launch_sequence_route": route[False]})
        print(json.dumps(rows[-1]), flush=True)
    os.environ.pop("HAMILTORCH_AMD_JIT", None)
    return {"device": torch.cuda.get_device_name(0), "warmup_calls": WARMUP, "timed_calls": TIMED, "rows": rows}


def resources():
    """vgpr / spill / scratch counts of the Metric.HESSIAN kernel around the log-cosh target at D = 1, 8, 16, both dtypes, jitter off and
    on - and of the soft-abs kernel (jitter on) around the same callable: the yardstick of the CPU test."""
    from hamiltorch_amd.jit import runtime
    from hamiltorch_amd.jit.trace import trace_callback

    def counts(Dk, dtype, jitter, metric):
        tr = trace_callback(logcosh(Dk), torch.ones(Dk, dtype=torch.float64))
        _, blob = runtime.compile_source(runtime.derivs_generated_source(tr, dtype, jitter, metric), runtime.SKELETON_RMHMC)
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob); f.flush()
            notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True).stdout
        keys = r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)"
        return dict({k: int(v) for k, v in re.findall(keys, notes)}, code_object_bytes=len(blob))

    out = []
    for Dk in (1, 8, 16):
        for dtype in (torch.float32, torch.float64):
            row = {"D": Dk, "dtype": runtime.dtype_name(dtype), "softabs_jitter1": counts(Dk, dtype, True, "softabs")}
            for jitter in (False, True):
                row["hessian_jitter%d" % jitter] = counts(Dk, dtype, jitter, "hessian")
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    mode = args.pop(0) if args and args[0] in ("rates", "resources") else "rates"
    out_dir = args[0] if args else os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, NAME)
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc["tool"] = "tools/jit_rmhmc_hessian_rate.py"
    if mode == "resources":
        doc["resources"] = resources()
    else:
        doc.update(rates())
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", path)
