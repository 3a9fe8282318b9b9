#!/usr/bin/env python
"""Rate of sample(sampler=RMHMC, integrator=IMPLICIT, metric=HESSIAN) on a general callable: the compiled trajectory kernel
(hta_cb_rmhmc_imp_hess_kernel, csrc/jit/rmhmc_implicit_callback.hip.in) against the launch sequence of the same library
(HAMILTORCH_AMD_JIT_IMPLICIT=0: compiled derivatives + one hta_metric_eval launch per evaluation + a host synchronisation per
fixed-point iteration - the route before the kernel existed), in one process - and the register / scratch counts of the kernel.

Workload: the log-cosh target (oracle.LogCoshTarget's form) at D = 8, float32, L = 10, eps = 0.1, jitter 1e-3, TRAJ trajectories per
call; 1024 and 65 536 chains; at sample()'s defaults (fixed_point_threshold 1e-5, fixed_point_max_iterations 1000: the loops end on
the threshold) and at leapfrog()'s (1e-20, 6: every iteration runs).  Protocol: modules built before timing, 2 warm-up calls, then the
median of 7 timed calls per route, each bracketed by device events around the whole sample() call - the end-of-run check of the
compiled route included, since every caller pays it.  The routes are alternated.  No rate is asked for: the number is the ratio, and
the compiled route is the default only while it beats the launch sequence at 1024 chains by more than the two spreads together.

    python tools/jit_rmhmc_implicit_rate.py [rates] [out_dir]      (needs the GPU)   "rows" of <out_dir or profiles>/r14a_rmhmc_implicit.json
    python tools/jit_rmhmc_implicit_rate.py resources [out_dir]    (hipRTC only)     "resources" of the same file: the counts
        tests/test_jit_rmhmc_implicit_cpu.py::test_resources_are_recorded looks for
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
D, L, EPS, JITTER, TRAJ = 8, 10, 0.1, 1e-3, 3
SETTINGS = (("sample() defaults", 1e-5, 1000), ("leapfrog() defaults", 1e-20, 6))
KERNEL = "hta_cb_rmhmc_imp_hess_kernel"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
NAME = "r14a_rmhmc_implicit.json"
HL2P = 0.9189385332046727


def logcosh(D):
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


def timed_call(ht, fn, th0, compiled, thr, max_it):
    from hamiltorch_amd import _abi
    os.environ["HAMILTORCH_AMD_JIT_IMPLICIT"] = "1" if compiled else "0"
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = ht.sample(fn, th0, num_samples=TRAJ, num_steps_per_sample=L, step_size=EPS, jitter=JITTER, fixed_point_threshold=thr,
                    fixed_point_max_iterations=max_it, sampler=ht.Sampler.RMHMC, integrator=ht.Integrator.IMPLICIT,
                    metric=ht.Metric.HESSIAN, verbose=False, seed=3)
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
        for name, thr, max_it in SETTINGS:
            secs, route = {True: [], False: []}, {}
            for compiled in (True, False):
                for _ in range(WARMUP):
                    timed_call(ht, fn, th0, compiled, thr, max_it)
            for _ in range(TIMED):
                for compiled in (True, False):
                    dt, route[compiled] = timed_call(ht, fn, th0, compiled, thr, max_it)
                    secs[compiled].append(dt)
            rate = {k: C * TRAJ * L / np.array(v) for k, v in secs.items()}
            med = {k: float(np.median(v)) for k, v in rate.items()}
            spread = {k: float((v.max() - v.min()) / np.median(v)) for k, v in rate.items()}
            # "beats by more than the two spreads together": the slowest compiled call against the fastest of the launch sequence
            clear = bool(med[True] * (1.0 - spread[True]) > med[False] * (1.0 + spread[False]))
            rows.append({"workload": "logcosh", "setting": name, "fixed_point_threshold": thr, "fixed_point_max_iterations": max_it, "D": D, "L": L,
                         "eps": EPS, "jitter": JITTER, "trajectories_per_call": TRAJ, "chains": C, "dtype": "f32",
                         "chain_steps_per_s": {"compiled": [float(x) for x in rate[True]], "launch_sequence": [float(x) for x in rate[False]]},
                         "median": {"compiled": med[True], "launch_sequence": med[False]}, "ratio": med[True] / med[False],
                         "spread": {"compiled": spread[True], "launch_sequence": spread[False]},
                         "compiled_is_faster_beyond_the_spreads": clear, "route": route[True], "launch_sequence_route": route[False]})
            print(json.dumps(rows[-1]), flush=True)
    os.environ.pop("HAMILTORCH_AMD_JIT_IMPLICIT", None)
    return {"device": torch.cuda.get_device_name(0), "warmup_calls": WARMUP, "timed_calls": TIMED, "rows": rows}


def resources():
    """vgpr / sgpr / spill / scratch counts of the float32 kernels (jitter on): Metric.HESSIAN around the log-cosh target at D = 8, the
    soft-abs one around the funnel at D = 5.  No bound goes with them: the explicit soft-abs kernel already spills by design."""
    from hamiltorch_amd.jit import runtime
    from hamiltorch_amd.jit.trace import trace_callback

    def counts(fn, Dk, metric):
        tr = trace_callback(fn, torch.ones(Dk, dtype=torch.float64))
        _, blob = runtime.compile_source(runtime.derivs_generated_source(tr, torch.float32, True, metric), runtime.SKELETON_RMHMC_IMPLICIT)
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob); f.flush()
            notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True).stdout
        keys = r"\.(vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)"
        return {k: int(v) for k, v in re.findall(keys, notes)}

    scales = np.array([0.5, 1.0, 1.7, 2.4])

    def scaled_funnel(w):
        s = torch.as_tensor(scales, dtype=w.dtype, device=w.device)
        v, x = w[0], w[1:]
        return -v * v / 18.0 - 1.0986122886681098 - HL2P + (-0.5 * torch.exp(v) * (x * x / s).sum() + 0.5 * x.numel() * v
                                                             - x.numel() * HL2P - 0.5 * torch.log(s).sum())
    out = {"hessian_D8_f32": counts(logcosh(8), 8, "hessian"), "softabs_D5_f32": counts(scaled_funnel, 5, "softabs")}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    mode = args.pop(0) if args and args[0] in ("rates", "resources") else "rates"
    out_dir = args[0] if args else os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, NAME)
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc["tool"] = "tools/jit_rmhmc_implicit_rate.py"
    if mode == "resources":
        doc["resources"] = resources()
    else:
        doc.update(rates())
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", path)
