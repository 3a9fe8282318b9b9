#!/usr/bin/env python
"""Time of hamiltorch_amd.diagnostics.summary against the host-driven path of hamiltorch_amd/ess.py (ess_min + rhat_max) on the same
seeded device tensors, at two shapes a user meets: [1000, 1024, 3] float32 (what BASELINE config 2 returns) and [200, 1024, 128]
float32 (the benchmark's slice of the notebook model).  Samples: AR(1) per coordinate, phi from 0 to 0.9 across d, in two variants:
"mixed" (stationary chains around one mean: the Geyer walks stop after a few dozen lags) and "offset" (every chain shifted by
0.3 N(0, 1): R-hat about 1.16, the between-chain term keeps rho positive and every walk runs to S - the most lags summary() computes).

    python tools/diag_rate.py rates <out_dir>            the two paths, 2 warm-up calls each per shape, then alternated REPS times, each
                                                         call between two device events, the second one synchronised (both paths end in
                                                         a host read); medians and spread.  Also checks that the two paths agree (1e-9).
    rocprofv3 --kernel-trace --stats -f csv -d <dir> -o k<i> -- python tools/diag_rate.py workload <i> <out_dir>
                                                         shape i alone ("offset" chains), CALLS summary() calls; writes the lag blocks it launched
    python tools/diag_rate.py report <tag> <out_dir>     merges the above with the kernels' registers / LDS / scratch (code-object
                                                         metadata of the built library) into <out_dir>/<tag>_diag_rate.json

The lag kernel's achieved bytes per second use its byte model - S C D itemsize per block of LAG_BLOCK lags - over the kernel time of
the rocprofv3 run, as a share of the 8.0 TB/s HBM peak.  (The samples of both shapes fit the 256 MiB Infinity Cache: the share says how
far the kernel is from a streaming bound, not that HBM delivered the bytes.)
"""
import csv
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hamiltorch_amd import _abi  # noqa: E402
from hamiltorch_amd import diagnostics as DG  # noqa: E402
from hamiltorch_amd import ess as E  # noqa: E402

SHAPES = [(1000, 1024, 3), (200, 1024, 128)]
WARMUP, REPS, CALLS = 2, 5, 5
HBM_PEAK = 8.0e12
LLVM = "/opt/rocm/lib/llvm/bin"


def make(shape, dev, chain_offset=0.3):
    S, C, D = shape
    g = torch.Generator(device="cpu").manual_seed(S * 7 + D)
    phi = torch.linspace(0.0, 0.9, D)
    e = torch.randn(S, C, D, generator=g)
    z = torch.empty(S, C, D)
    z[0] = e[0]
    for s in range(1, S):
        z[s] = phi * z[s - 1] + torch.sqrt(1.0 - phi * phi) * e[s]
    return (torch.linspace(0.5, 3.0, D) * z + torch.linspace(-100.0, 100.0, D) + chain_offset * torch.randn(C, D, generator=g)).to(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def rates(out_dir):
    dev = torch.device("cuda:0")
    rows = []
    for shape, variant in [(sh, v) for sh in SHAPES for v in ("mixed", "offset")]:
        x = make(shape, dev, 0.0 if variant == "mixed" else 0.3)
        new = lambda: (lambda s: (s.min_ess(), s.max_rhat()))(DG.summary(x))       # noqa: E731
        old = lambda: (E.ess_min(x), E.rhat_max(x))                                 # noqa: E731
        for fn in (new, old):
            for _ in range(WARMUP):
                timed(fn)
        secs = {"summary": [], "ess_py": []}
        for _ in range(REPS):
            dt, got = timed(new)
            secs["summary"].append(dt)
            dt, ref = timed(old)
            secs["ess_py"].append(dt)
        agree = max(abs(got[0] - ref[0]) / ref[0], abs(got[1] - ref[1]) / ref[1])
        med = {k: float(np.median(v)) for k, v in secs.items()}
        rows.append({"shape": list(shape), "dtype": "f32", "chains": variant, "seconds": secs, "median_seconds": med,
                     "spread": {k: float((max(v) - min(v)) / np.median(v)) for k, v in secs.items()},
                     "speedup": med["ess_py"] / med["summary"], "summary_is_faster": bool(med["summary"] < med["ess_py"]),
                     "ess_min": got[0], "rhat_max": got[1], "max_lags_used": int(DG.summary(x).lags_used.max()), "relative_difference_to_ess_py": agree, "route": _abi.last_route()})
        assert agree <= 1e-9, rows[-1]
        print(json.dumps(rows[-1]), flush=True)
    with open(os.path.join(out_dir, "diag_rates.json"), "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "warmup_calls": WARMUP, "alternated_calls": REPS, "rows": rows}, f, indent=1)


class _Counting:
    """The library with the lag blocks of hta_diag_lags_* counted."""

    def __init__(self, lib):
        self.lib, self.blocks, self.launches = lib, 0, 0

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("hta_diag_lags_"):
            return fn

        def counted(*a):
            self.blocks += int(a[7]) // DG.LAG_BLOCK
            self.launches += 1
            return fn(*a)
        return counted


def workload(i, out_dir):
    dev = torch.device("cuda:0")
    shape = SHAPES[i]
    x = make(shape, dev)
    lib = _Counting(_abi.load())
    _abi.load = lambda: lib
    for _ in range(CALLS):
        s = DG.summary(x)
    torch.cuda.synchronize()
    with open(os.path.join(out_dir, "diag_workload_%d.json" % i), "w") as f:
        json.dump({"shape": list(shape), "itemsize": x.element_size(), "calls": CALLS, "lag_blocks": lib.blocks, "lag_launches": lib.launches,
                   "max_lags_used": int(s.lags_used.max())}, f)


def code_objects():
    """registers / LDS / scratch of the diagnostics kernels from the built library's code-object metadata."""
    import tempfile
    lib = os.path.join(ROOT, "hamiltorch_amd", "libhamiltorch_amd.so")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["cp", lib, os.path.join(d, "lib.so")], check=True)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], cwd=d, check=True, capture_output=True, text=True).stdout
            for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk)
                if not name or "diag_" not in name.group(1):
                    continue
                g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))      # noqa: E731
                out[name.group(1)] = {"vgpr": g("vgpr_count"), "sgpr": g("sgpr_count"), "lds_bytes": g("group_segment_fixed_size"),
                                      "scratch_bytes": g("private_segment_fixed_size"), "vgpr_spills": g("vgpr_spill_count")}
    return out


def report(tag, out_dir):
    res = json.load(open(os.path.join(out_dir, "diag_rates.json")))
    kernels = []
    for i, shape in enumerate(SHAPES):
        w = json.load(open(os.path.join(out_dir, "diag_workload_%d.json" % i)))
        stats = {}
        for p in glob.glob(os.path.join(out_dir, "**", "*k%d_kernel_stats.csv" % i), recursive=True):
            for r in csv.DictReader(open(p)):
                if "diag_" in r["Name"]:
                    stats[re.sub(r"^void hta::|\(.*$", "", r["Name"])] = {"calls": int(r["Calls"]), "total_ns": int(r["TotalDurationNs"])}
        lag = next(v for k, v in stats.items() if k.startswith("diag_lags_kernel"))
        S, C, D = shape
        model = w["lag_blocks"] * S * C * D * w["itemsize"]
        rate = model / (lag["total_ns"] * 1e-9)
        kernels.append({"shape": shape, "summary_calls": w["calls"], "lag_blocks": w["lag_blocks"], "lag_launches": w["lag_launches"],
                        "max_lags_used": w["max_lags_used"], "kernel_stats": stats, "lag_kernel_model_bytes": model,
                        "lag_kernel_bytes_per_s": rate, "lag_kernel_share_of_hbm_peak": rate / HBM_PEAK})
    res.update({"tool": "tools/diag_rate.py", "hbm_peak_bytes_per_s": HBM_PEAK, "byte_model": "S C D itemsize per block of LAG_BLOCK lags",
                "lag_block": DG.LAG_BLOCK, "segment_rows": DG.SEGMENT_ROWS, "kernel_trace": kernels, "code_objects": code_objects()})
    path = os.path.join(out_dir, "%s_diag_rate.json" % tag)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "rates":
        os.makedirs(sys.argv[2], exist_ok=True)
        rates(sys.argv[2])
    elif mode == "workload":
        os.makedirs(sys.argv[3], exist_ok=True)
        workload(int(sys.argv[2]), sys.argv[3])
    elif mode == "report":
        report(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
