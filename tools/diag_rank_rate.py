#!/usr/bin/env python
"""Time of hamiltorch_amd.diagnostics.rank_summary against the same quantities composed from torch on the same seeded device tensors,
at the two shapes of tools/diag_rate.py - [1000, 1024, 3] and [200, 1024, 128] float32, "mixed" chains (stationary AR(1) chains around
one mean).  The torch composition, per coordinate: torch.sort of the S C draws, the tie runs by unique_consecutive, the average ranks
scattered back through the permutation, torch.special.ndtri in float64, the same for |x - median|, the indicators and the quantiles
from the sorted draws; then summary() on the derived series (z, I05, I95; the moments of zf), as rank_summary() does.

    python tools/diag_rank_rate.py rates <out_dir>       the two paths, 2 warm-up calls each per shape, then alternated REPS times, each
                                                         call between two device events, the second one synchronised (both paths end in
                                                         a host read); medians and spread.  Also checks that the two paths agree (1e-9).
    rocprofv3 --kernel-trace --stats -f csv -d <dir> -o k<i> -- python tools/diag_rank_rate.py workload <i> <out_dir>
                                                         shape i alone, CALLS rank_summary() calls
    python tools/diag_rank_rate.py report <tag> <out_dir>   merges the above with the kernels' registers / LDS / scratch (code-object
                                                         metadata of the built library) into <out_dir>/<tag>_diag_rank_rate.json

Byte models per call of rank_summary() (N = S C draws, D coordinates, kb = key bytes, 4-byte payloads; a first sort of kb = 4 for
float32 samples and the fold's sort of kb = 8, so 12 passes of 8 bits): the histogram kernel reads the keys once per pass, the scatter
kernel reads and writes keys and payloads once per pass, the scan kernel reads and writes 256 counts per tile twice.  Achieved bytes
per second = model bytes over the kernel's time in the rocprofv3 run, as a share of the 8.0 TB/s HBM peak (both shapes fit the 256 MiB
Infinity Cache: the share says how far a kernel is from a streaming bound, not that HBM delivered the bytes).
"""
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hamiltorch_amd import diagnostics as DG  # noqa: E402
from diag_rate import CALLS, HBM_PEAK, REPS, SHAPES, WARMUP, code_objects, make, timed  # noqa: E402

FIELDS = ("ess_bulk", "ess_tail", "rhat", "rhat_bulk", "rhat_folded", "q05", "median", "q95")


def _scores(v):
    """v[N] -> (normal scores of the average ranks [N] float64, the sorted values)."""
    N = v.numel()
    srt, perm = torch.sort(v)
    _, inverse, counts = torch.unique_consecutive(srt, return_inverse=True, return_counts=True)
    ends = torch.cumsum(counts, 0).to(torch.float64)
    avg = ends - (counts.to(torch.float64) - 1.0) * 0.5
    r = torch.empty(N, dtype=torch.float64, device=v.device)
    r[perm] = avg[inverse]
    return torch.special.ndtri((r - 0.375) / (N + 0.25)), srt


def _quantile(srt, q):
    N = srt.numel()
    h = (N - 1) * q
    lo = int(np.floor(h))
    a, b = srt[lo].double(), srt[min(lo + 1, N - 1)].double()
    return a + (b - a) * (h - lo)


def torch_rank_summary(x):
    """rank_summary(x) from torch ops and summary(): x[S, C, D] on the device -> dict of [D] float64 tensors."""
    S, C, D = x.shape
    N = S * C
    f64 = dict(dtype=torch.float64, device=x.device)
    z, zf = torch.empty(S, C, D, **f64), torch.empty(S, C, D, **f64)
    i05, i95 = (torch.empty(S, C, D, dtype=torch.float32, device=x.device) for _ in range(2))
    q = torch.empty(3, D, **f64)
    for d in range(D):
        col = x[:, :, d].reshape(N)
        zd, srt = _scores(col)
        z[:, :, d] = zd.view(S, C)
        med = 0.5 * (srt[(N - 1) // 2].double() + srt[N // 2].double())
        zf[:, :, d] = _scores((col.double() - med).abs())[0].view(S, C)
        i05[:, :, d] = (col <= srt[(N - 1) // 20]).view(S, C)
        i95[:, :, d] = (col <= srt[19 * (N - 1) // 20]).view(S, C)
        q[0, d], q[1, d], q[2, d] = _quantile(srt, 0.05), _quantile(srt, 0.5), _quantile(srt, 0.95)
    sz = DG.summary(z)
    rf = DG.summary(zf, max_lag=DG.LAG_BLOCK).rhat
    return {"ess_bulk": sz.ess_bulk, "ess_tail": torch.minimum(DG.summary(i05).ess_bulk, DG.summary(i95).ess_bulk), "rhat": torch.maximum(sz.rhat, rf),
            "rhat_bulk": sz.rhat, "rhat_folded": rf, "q05": q[0], "median": q[1], "q95": q[2]}


def _read(d):
    """the host read both paths end in: min over both ESS fields, max R-hat."""
    return float(torch.minimum(d["ess_bulk"], d["ess_tail"]).min()), float(d["rhat"].max())


def rates(out_dir):
    dev = torch.device("cuda:0")
    rows = []
    for shape in SHAPES:
        x = make(shape, dev, 0.0)
        new = lambda: (lambda s: ((s.min_ess(), s.max_rhat()), s))(DG.rank_summary(x))                       # noqa: E731
        old = lambda: (lambda d: (_read(d), d))(torch_rank_summary(x))                                        # noqa: E731
        for fn in (new, old):
            for _ in range(WARMUP):
                timed(fn)
        secs = {"rank_summary": [], "torch": []}
        for _ in range(REPS):
            dt, (got, s) = timed(new)
            secs["rank_summary"].append(dt)
            dt, (ref, t) = timed(old)
            secs["torch"].append(dt)
        # (relative; the quantiles against |q| + 1: a median may be near zero and the draws' scales are 0.5 to 3)
        agree = max(float(((getattr(s, f) - t[f]).abs() / (t[f].abs() + (1.0 if f in ("q05", "median", "q95") else 0.0))).max()) for f in FIELDS)
        med = {k: float(np.median(v)) for k, v in secs.items()}
        spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in secs.items()}
        rows.append({"shape": list(shape), "dtype": "f32", "chains": "mixed", "seconds": secs, "median_seconds": med, "spread": spread,
                     "speedup": med["torch"] / med["rank_summary"], "rank_summary_is_faster": bool(med["rank_summary"] < med["torch"]),
                     "slower_by_more_than_the_spread": bool(med["rank_summary"] > med["torch"] * (1.0 + max(spread.values()))),
                     "min_ess": got[0], "max_rhat": got[1], "relative_difference_to_torch": agree, "chunks": len(DG.rank_plan(*shape).chunks), "route": s.route})
        assert agree <= 1e-9 and abs(got[0] - ref[0]) <= 1e-9 * ref[0], rows[-1]
        print(json.dumps(rows[-1]), flush=True)
    with open(os.path.join(out_dir, "diag_rank_rates.json"), "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "warmup_calls": WARMUP, "alternated_calls": REPS, "rows": rows}, f, indent=1)


def workload(i, out_dir):
    dev = torch.device("cuda:0")
    shape = SHAPES[i]
    x = make(shape, dev, 0.0)
    for _ in range(CALLS):
        s = DG.rank_summary(x)
    torch.cuda.synchronize()
    with open(os.path.join(out_dir, "diag_rank_workload_%d.json" % i), "w") as f:
        json.dump({"shape": list(shape), "itemsize": x.element_size(), "calls": CALLS, "chunks": len(DG.rank_plan(*shape).chunks), "min_ess": s.min_ess()}, f)


def byte_models(shape, itemsize):
    """model bytes per rank_summary() call and kernel (see the module docstring)."""
    S, C, D = shape
    N = S * C
    tiles = -(-N // DG.RANK_TILE)
    out = {"diag_rank_hist_kernel": 0, "diag_rank_scan_kernel": 0, "diag_rank_scatter_kernel": 0}
    for kb in (itemsize, 8):                                       # the first sort, the fold's sort
        out["diag_rank_hist_kernel"] += kb * N * D * kb
        out["diag_rank_scatter_kernel"] += kb * 2 * N * D * (kb + 4)
        out["diag_rank_scan_kernel"] += kb * 4 * D * tiles * 256 * 4
    out["diag_rank_gather_kernel"] = N * D * (itemsize + itemsize + 4) + N * D * (itemsize + 8 + 4)
    out["diag_rank_transform_kernel"] = N * D * (itemsize + 4 + 8 + 4 + 4) + N * D * (8 + 4 + 8)
    return out


def report(tag, out_dir):
    res = json.load(open(os.path.join(out_dir, "diag_rank_rates.json")))
    kernels = []
    for i, shape in enumerate(SHAPES):
        w = json.load(open(os.path.join(out_dir, "diag_rank_workload_%d.json" % i)))
        stats = {}
        for p in glob.glob(os.path.join(out_dir, "**", "*k%d_kernel_stats.csv" % i), recursive=True):
            for r in csv.DictReader(open(p)):
                if "diag_" in r["Name"]:
                    stats[re.sub(r"^(void )?hta::|\(.*$", "", r["Name"])] = {"calls": int(r["Calls"]), "total_ns": int(r["TotalDurationNs"])}
        model = byte_models(shape, w["itemsize"])
        per_kernel = {}
        for name, nbytes in model.items():
            ns = sum(v["total_ns"] for k, v in stats.items() if k.startswith(name))
            launches = sum(v["calls"] for k, v in stats.items() if k.startswith(name))
            rate = nbytes * w["calls"] / (ns * 1e-9) if ns else None
            per_kernel[name] = {"launches_per_call": launches / w["calls"], "ms_per_call": ns * 1e-6 / w["calls"], "model_bytes_per_call": nbytes,
                                "bytes_per_s": rate, "share_of_hbm_peak": rate / HBM_PEAK if rate else None}
        rank_ns = sum(v["total_ns"] for k, v in stats.items() if k.startswith("diag_rank_"))
        rest_ns = sum(v["total_ns"] for k, v in stats.items() if not k.startswith("diag_rank_"))
        kernels.append({"shape": shape, "rank_summary_calls": w["calls"], "chunks": w["chunks"], "kernel_stats": stats, "rank_kernels": per_kernel,
                        "rank_kernels_ms_per_call": rank_ns * 1e-6 / w["calls"], "existing_stages_ms_per_call": rest_ns * 1e-6 / w["calls"]})
    res.update({"tool": "tools/diag_rank_rate.py", "hbm_peak_bytes_per_s": HBM_PEAK,
                "byte_model": "per 8-bit pass: hist reads the keys, scatter reads and writes keys and 4-byte payloads, scan reads and writes 256 counts per tile twice",
                "rank_tile": DG.RANK_TILE, "kernel_trace": kernels, "code_objects": {k: v for k, v in code_objects().items() if "diag_rank_" in k}})
    path = os.path.join(out_dir, "%s_diag_rank_rate.json" % tag)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
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
