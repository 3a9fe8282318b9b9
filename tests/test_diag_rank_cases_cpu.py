"""No GPU: what tests/test_gpu_diag_rank.py takes for granted about tests/diag_rank_cases.py - the table reaches every edge, the
index form of the tail indicators is numpy's quantile form, and no Geyer walk of a derived series (z, I05, I95) passes within 1e-6 of a
zero pair sum, so lags can be compared exactly and ESS at 1e-9 - and the parts of the rank-normalised diagnostics that need no device:
the planner, the argument errors, the exports, the host build of the device's Phi^-1 and the resources of the built kernels."""
import numpy as np
import pytest
import torch

import diag_rank_cases as R
from hamiltorch_amd import diagnostics as DG


def test_the_table_reaches_every_edge():
    T = R.T
    long_chain = {c.S for c in R.CASES if c.C == 1}
    assert long_chain == {4, 5, T - 1, T, T + 1, 2 * T + 3}
    short = {c.S * c.C for c in R.CASES if c.S in (4, 5) and c.C > 1}
    assert {T - 3, T, T + 2, 2 * T + 4} <= short                                   # S = 4 or 5 on both sides of every tile edge
    assert {T - 1, T + 1} <= {c.S * c.C for c in R.CASES if c.C > 1}               # and the edges themselves with several chains
    assert any(abs(c.S * c.C - 70 * 257) <= 10 for c in R.CASES)
    assert {c.D for c in R.CASES} == {1, 3, 67, 130}
    assert {c.variant for c in R.CASES} == set("abcde")
    for v in "abcd":
        assert {c.dtype for c in R.CASES if c.variant == v} == {np.float32, np.float64}, v
    assert {c.dtype for c in R.CASES if c.variant == "e"} == {np.float64}
    for D in (1, 3, 67, 130):
        assert {c.dtype for c in R.CASES if c.D == D} == {np.float32, np.float64}, D
    assert len(set(R.IDS)) == len(R.IDS) <= 32


def test_constants_are_the_library_s():
    from hamiltorch_amd import _abi
    lib = _abi.load()
    assert lib.hta_diag_rank_tile() == DG.RANK_TILE and DG.RANK_TILE % 256 == 0
    for S, C, D, kb in ((4, 1, 1, 4), (257, 70, 5, 8), (1000, 1024, 3, 8), (200, 300, 129, 4), (5, 3598, 3, 8)):
        assert lib.hta_diag_rank_workspace_bytes(S, C, D, kb) == DG.rank_workspace_bytes_for(S, C, D, kb), (S, C, D, kb)
    assert lib.hta_diag_rank_workspace_bytes(1 << 16, 1 << 15, 1, 8) == -1          # S C = 2^31
    assert lib.hta_diag_rank_workspace_bytes(4, 1, 1, 2) == -1


def test_the_variants_hold_what_they_promise():
    for c in R.CASES:
        x = R.samples(c)
        assert x.dtype == c.dtype and x.shape == (c.S, c.C, c.D)
        col = x[:, :, 0].ravel()
        if c.variant == "b":
            _, counts = np.unique(col, return_counts=True)
            assert np.array_equal(col * 2, np.round(col * 2)) and (c.S * c.C < 100 or counts.max() >= 100)
        if c.variant == "c":
            assert np.signbit(col[col == 0]).any() and not np.signbit(col[col == 0]).all()
            assert (col < 0).any() and ((col != 0) & (np.abs(col) < np.finfo(np.float32).tiny)).any()
            one = c.dtype(1.0)
            assert (col == one).any() and (col == np.nextafter(one, c.dtype(2.0))).any()
        if c.variant == "d":
            assert np.all(x[:, :, R.CONSTANT] == 2.5) and np.isnan(x[:, :, R.WITH_NAN]).sum() == 1 and np.isinf(x[:, :, R.WITH_INF]).sum() == 1
        if c.variant == "e":
            assert len(np.unique(col)) > 0.9 * col.size and len(np.unique(col.astype(np.float32))) <= 3


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_reference_and_guard(case):
    """the index form of the indicators is numpy's quantile form; the degenerate coordinates are NaN and only they (a constant tail
    indicator aside); every pair sum on a walk of z, I05, I95 is at least 1e-6 from zero."""
    x = R.samples(case)
    r = R.referenced(case)
    x64 = x.astype(np.float64)
    N = case.S * case.C
    for d in range(case.D):
        col = x64[:, :, d]
        if not np.isfinite(col).all():
            continue
        assert np.array_equal(r.i05[:, :, d], col <= np.quantile(col, 0.05)), d
        assert np.array_equal(r.i95[:, :, d], col <= np.quantile(col, 0.95)), d
        srt = np.sort(col.ravel())
        assert abs(r.median[d] - 0.5 * (srt[(N - 1) // 2] + srt[N // 2])) <= 1e-15 * abs(r.median[d])
    bad = [R.CONSTANT, R.WITH_NAN, R.WITH_INF] if case.variant == "d" else []
    for f in ("ess_bulk", "rhat", "rhat_bulk", "rhat_folded"):
        v = getattr(r, f)
        assert np.array_equal(np.flatnonzero(np.isnan(v)), bad), f
    for f in ("q05", "median", "q95"):
        assert np.array_equal(np.flatnonzero(np.isnan(getattr(r, f))), bad[1:]), f
    if bad:
        assert r.q05[R.CONSTANT] == r.median[R.CONSTANT] == r.q95[R.CONSTANT] == 2.5
    constant_tail = [d for d in range(case.D) if d not in bad and (r.i05[:, :, d].min() == r.i05[:, :, d].max() or r.i95[:, :, d].min() == r.i95[:, :, d].max())]
    assert np.array_equal(np.flatnonzero(np.isnan(r.ess_tail)), sorted(bad + constant_tail))
    assert case.variant == "b" or not constant_tail
    assert np.nanmin(r.small) >= 1e-6, np.nanmin(r.small)


def test_zeros_tie_in_the_reference():
    case = next(c for c in R.CASES if c.variant == "c" and c.dtype == np.float32)
    x, r = R.samples(case), R.referenced(case)
    z = r.z[:, :, 0][x[:, :, 0] == 0]
    assert z.size >= 2 and np.all(z == z[0])


def test_host_build_of_the_normal_quantile():
    """AS 241 PPND16 as compiled for the host against scipy's ndtri on every p that (r - 3/8) / (N + 1/4) can take for N < 2^31."""
    from scipy import special
    from hamiltorch_amd import _abi
    lib = _abi.load()
    lo = 0.625 / (2.0 ** 31 + 0.25)
    p = np.concatenate([[6e-8, 1 - 6e-8, lo, 1 - lo, 0.5, 0.075, 0.925], np.linspace(1e-9, 1 - 1e-9, 4001), np.logspace(np.log10(lo), -1, 1000)])
    got = np.array([lib.hta_diag_rank_ndtri(float(v)) for v in p])
    ref = special.ndtri(p)
    err = np.abs(got - ref) / np.where(ref == 0, 1.0, np.abs(ref))
    assert err.max() <= 4e-15, (err.max(), p[err.argmax()])
    assert lib.hta_diag_rank_ndtri(0.5) == 0.0


# ---- the planner ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,D,cap", [(200, 1024, 128, 256 << 20), (200, 1024, 128, 16 << 20), (1000, 1024, 3, 256 << 20), (515, 70, 130, 8 << 20),
                                       (257, 3, 130, 400_000), (4, 1, 1, 1 << 11), (5000, 64, 1000, 64 << 20)])
def test_rank_plan_covers_every_coordinate_once_under_the_cap(S, C, D, cap):
    p = DG.rank_plan(S, C, D, 4, cap)
    assert p.chunks[0][0] == 0 and p.chunks[-1][1] == D
    assert all(a < b for a, b in p.chunks) and all(p.chunks[i][1] == p.chunks[i + 1][0] for i in range(len(p.chunks) - 1))
    assert all(DG.rank_bytes_for(S, C, b - a, p.lags_per_launch) <= cap for a, b in p.chunks)
    assert p.n_tiles == -(-(S * C) // DG.RANK_TILE) and p.lags_per_launch == DG.plan(S, C, 1).lags_per_launch
    assert (p.chunks == [(0, D)]) == (DG.rank_bytes_for(S, C, D, p.lags_per_launch) <= cap)


def test_rank_plan_counts_every_buffer():
    S, C, D = 257, 3, 130
    n_lags = DG.plan(S, C, D).lags_per_launch
    one = DG.rank_bytes_for(S, C, 1, n_lags)
    N = S * C
    assert one == 2 * (-(-N * 8 // 8) * 8) + 2 * (-(-N * 4 // 8) * 8) + 1024 + 16 * N + DG.workspace_bytes_for(S, C, 1, n_lags)
    assert len(DG.rank_plan(S, C, D, 8, 50 * one).chunks) >= 3
    assert len(DG.rank_plan(S, C, D, 8, one + 8).chunks) == D


def test_rank_plan_refuses_a_cap_below_one_coordinate():
    one = DG.rank_bytes_for(1000, 1024, 1, DG.plan(1000, 1024, 3).lags_per_launch)
    assert DG.rank_plan(1000, 1024, 3, 4, one).chunks == [(0, 1), (1, 2), (2, 3)]
    with pytest.raises(ValueError, match="cannot hold one coordinate"):
        DG.rank_plan(1000, 1024, 3, 4, one - 1)
    with pytest.raises(ValueError, match="2\\^31"):
        DG.rank_plan(1 << 16, 1 << 15, 3)


# ---- argument errors: raised before anything touches a device ------------------------------------------------------------------------
def test_argument_errors(monkeypatch):
    from hamiltorch_amd import _abi
    monkeypatch.setattr(_abi, "load", lambda: pytest.fail("rank_summary() reached the library"))
    monkeypatch.setattr(_abi, "require_device", lambda *a, **k: pytest.fail("rank_summary() reached the device check"))
    x = torch.zeros(8, 2, 3)
    with pytest.raises(ValueError, match="at least 4"):
        DG.rank_summary(x[:3])
    with pytest.raises(ValueError, match="at least 4"):
        DG.rank_summary(x, skip=5)
    with pytest.raises(ValueError, match="at least 4"):
        DG.ess_tail([r for r in x[:4]], skip=1)
    with pytest.raises(ValueError, match="floating point"):
        DG.rank_summary(torch.zeros(8, 2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="floating point"):
        DG.rhat_rank(torch.zeros(8, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\[S, C, D\]"):
        DG.rank_summary(torch.zeros(8))
    with pytest.raises(ValueError, match="max_lag"):
        DG.rank_summary(x, max_lag=1)
    with pytest.raises(ValueError, match="cannot hold one coordinate"):
        DG.rank_summary(x, workspace_bytes=64)
    with pytest.raises(ValueError, match="2\\^31"):                               # refused by shape arithmetic: nothing this size is allocated
        DG.rank_summary(torch.zeros(1, dtype=torch.float32).expand(1 << 16, 1 << 15, 1))


def test_the_library_refuses_bad_arguments_without_a_device():
    """before any launch, and so also where there is no GPU: shape, S C >= 2^31, strides, workspace."""
    import ctypes
    from hamiltorch_amd import _abi
    lib = _abi.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rank = lambda *a: lib.hta_diag_rank_f32(p, *a, p, p, p, p, p, p, p, p, p, 1 << 40, None)      # noqa: E731
    assert rank(6, 3, 3, 2, 3) == -1 and b"bad shape" in lib.hta_last_error()
    assert rank(1 << 15, 1, 1 << 16, 1 << 15, 1) == -1 and b"bad shape" in lib.hta_last_error()
    assert rank(6, 2, 8, 2, 3) == -1 and b"bad strides" in lib.hta_last_error()
    assert lib.hta_diag_rank_f32(p, 6, 3, 8, 2, 3, p, p, p, p, p, p, p, p, p, 64, None) == -1 and b"workspace" in lib.hta_last_error()
    assert lib.hta_diag_rank_folded_f64(p, 6, 3, 8, 2, 3, p, p, p, p, 64, None) == -1 and b"workspace" in lib.hta_last_error()
    assert lib.hta_diag_rank_folded_f64(p, 6, 3, 8, 2, 3, None, p, p, p, 1 << 40, None) == -1 and b"NULL" in lib.hta_last_error()


def test_module_exports_the_rank_names():
    import hamiltorch_amd
    assert hamiltorch_amd.diagnostics is DG
    for name in ("rank_summary", "RankSummary", "ess_tail", "rhat_rank", "rank_plan", "RANK_TILE"):
        assert hasattr(DG, name), name
    from hamiltorch_amd import _abi
    assert {"hta_diag_rank", "hta_diag_rank_folded"} <= set(_abi.TYPED_SYMBOLS) and "hta_diag_rank_workspace_bytes" in _abi.PLAIN_SYMBOLS
    assert _abi.ABI_VERSION == 17


# ---- the built kernels --------------------------------------------------------------------------------------------------------------
def test_no_scratch_and_no_spills_in_the_rank_kernels(tmp_path):
    """the gfx950 code objects of csrc/diagnostics_rank.hip: every instance of every kernel is there, none spills or uses scratch."""
    import os
    import re
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    llvm = "/opt/rocm/lib/llvm/bin"
    shutil.copy(os.path.join(root, "hamiltorch_amd", "libhamiltorch_amd.so"), tmp_path / "lib.so")
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp_path, check=True, capture_output=True)
    found = {}
    for f in sorted(os.listdir(tmp_path)):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", f], cwd=tmp_path, check=True, capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if name and "diag_rank_" in name.group(1):
                g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))      # noqa: E731
                found[name.group(1)] = (g("vgpr_count"), g("private_segment_fixed_size"), g("vgpr_spill_count"), g("sgpr_spill_count"))
    for part, instances in (("diag_rank_gather_kernel", 4), ("diag_rank_hist_kernel", 2), ("diag_rank_scan_kernel", 1), ("diag_rank_scatter_kernel", 2),
                            ("diag_rank_transform_kernel", 3)):
        hits = [k for k in found if part in k]
        assert len(hits) == instances, (part, sorted(found))
        for k in hits:
            assert found[k][1:] == (0, 0, 0), (k, found[k])
