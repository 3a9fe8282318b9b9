"""No GPU: what tests/test_gpu_diagnostics.py takes for granted about tests/diag_cases.py - the numpy restatement by direct summation
agrees with the oracle's FFT form and with ess.py on every case, no Geyer walk of the table passes close enough to a zero pair sum
for a reordered fp64 sum to move its truncation point, both endings of the walk occur - and the parts of hamiltorch_amd/diagnostics.py
that need no device: the workspace planner and the argument errors."""
import numpy as np
import pytest
import torch

import diag_cases as T
from hamiltorch_amd import diagnostics as DG


def test_the_table_reaches_every_edge():
    B, R = T.B, T.R
    assert {c.S for c in T.CASES} == {4, 5, B, B + 1, 2 * B + 1, R - 1, R, R + 1, 2 * R + 3}
    assert {c.C for c in T.CASES} == {1, 3, 64, 70}
    assert {c.D for c in T.CASES} == {1, 3, 5, 67, 130}
    for axis in ("S", "C", "D"):
        for v in {getattr(c, axis) for c in T.CASES}:
            assert {c.dtype for c in T.CASES if getattr(c, axis) == v} == {np.float32, np.float64}, (axis, v)
    assert 24 <= len(T.CASES) <= 48 and len(set(T.IDS)) == len(T.IDS)


def test_constants_are_the_library_s():
    from hamiltorch_amd import _abi
    lib = _abi.load()
    assert (lib.hta_diag_lag_block(), lib.hta_diag_segment_rows()) == (DG.LAG_BLOCK, DG.SEGMENT_ROWS)
    for S, C, D, n in ((4, 1, 1, 0), (257, 70, 5, 272), (1000, 1024, 3, 512), (200, 300, 129, 208)):
        assert lib.hta_diag_workspace_bytes(S, C, D, n) == DG.workspace_bytes_for(S, C, D, n), (S, C, D, n)


@pytest.mark.parametrize("case", T.CASES, ids=T.IDS)
def test_restatement_agrees_with_the_oracle_and_ess_py(case):
    """the guard of the GPU test: 1e-9 between direct summation and the FFT form (the tolerance tests/test_host_logic.py uses between
    ess.py and the oracle), 1e-12 for R-hat, and every pair sum on a walk at least 1e-6 from zero."""
    from hamiltorch_amd import ess as E
    r, ref = T.restated(case), T.reference(case)
    x = T.samples(case)
    assert x.dtype == case.dtype and x.shape == (case.S, case.C, case.D)
    assert np.all(np.isfinite(r.ess)) and np.all(np.isfinite(r.rhat))
    np.testing.assert_allclose(r.ess, ref.ess, rtol=1e-9, atol=0)
    np.testing.assert_allclose(r.rhat, ref.rhat, rtol=1e-12, atol=0)
    assert r.small.min() >= 1e-6, r.small.min()
    xt = torch.from_numpy(x)
    d = case.D // 2
    assert abs(E.ess_bulk(xt[:, :, d]) - r.ess[d]) <= 1e-9 * r.ess[d]
    assert np.all(r.own)                                           # without max_lag every walk ends by itself
    assert np.all(r.lags % 2 == 0) and np.all(r.lags <= case.S)


def test_both_endings_of_the_walk_occur():
    early = sum(int(((T.restated(c).lags + 1 < c.S)).sum()) for c in T.CASES)
    to_the_end = [(c, d) for c in T.CASES if c.S >= 2 * T.B + 1 for d in range(c.D) if T.restated(c).lags[d] + 1 >= c.S]
    assert early > 0 and to_the_end, (early, len(to_the_end))


def test_walk_stopped_by_max_lag():
    case, d = T.run_to_the_end_case()
    x = T.samples(case)
    full, cut = T.restated(case), T.restate(x, max_lag=T.B)
    assert full.own[d] and not cut.own[d] and cut.lags[d] == T.B and cut.tau[d] < full.tau[d]


# ---- the planner ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,D,cap", [(200, 1024, 128, 256 << 20), (200, 1024, 128, 16 << 20), (1000, 1024, 3, 256 << 20), (515, 70, 130, 3 << 20),
                                       (257, 3, 130, 400_000), (4, 1, 1, 1 << 10), (5000, 64, 1000, 64 << 20)])
def test_plan_covers_every_coordinate_once_under_the_cap(S, C, D, cap):
    p = DG.plan(S, C, D, 4, cap)
    assert p.chunks[0][0] == 0 and p.chunks[-1][1] == D
    assert all(a < b for a, b in p.chunks) and all(p.chunks[i][1] == p.chunks[i + 1][0] for i in range(len(p.chunks) - 1))
    assert all(DG.workspace_bytes_for(S, C, b - a, p.lags_per_launch) <= cap for a, b in p.chunks)
    assert p.n_segments == -(-S // DG.SEGMENT_ROWS) and p.chain_groups == min(C, DG.CHAIN_GROUPS)
    assert p.lags_per_launch % DG.LAG_BLOCK == 0 and 0 < p.lags_per_launch <= DG.LAG_BLOCK * DG.MAX_LAG_BLOCKS
    if DG.workspace_bytes_for(S, C, D, p.lags_per_launch) <= cap:
        assert p.chunks == [(0, D)]
    else:
        assert len(p.chunks) >= 2


def test_plan_chunk_counts():
    S, C, D = 257, 3, 130
    one = DG.workspace_bytes_for(S, C, 1, DG.plan(S, C, D).lags_per_launch)
    assert len(DG.plan(S, C, D, 8, 50 * one).chunks) >= 3
    assert len(DG.plan(S, C, D, 8, one + 8).chunks) == D


def test_plan_refuses_a_cap_below_one_coordinate():
    one = DG.workspace_bytes_for(1000, 1024, 1, DG.plan(1000, 1024, 3).lags_per_launch)
    assert DG.plan(1000, 1024, 3, 4, one).chunks == [(0, 1), (1, 2), (2, 3)]
    with pytest.raises(ValueError, match="cannot hold one coordinate"):
        DG.plan(1000, 1024, 3, 4, one - 1)


# ---- argument errors: raised before anything touches a device ------------------------------------------------------------------------
def test_argument_errors(monkeypatch):
    from hamiltorch_amd import _abi
    monkeypatch.setattr(_abi, "load", lambda: pytest.fail("summary() reached the library"))
    monkeypatch.setattr(_abi, "require_device", lambda *a, **k: pytest.fail("summary() reached the device check"))
    x = torch.zeros(8, 2, 3)
    with pytest.raises(ValueError, match="at least 4"):
        DG.summary(x[:3])
    with pytest.raises(ValueError, match="at least 4"):
        DG.summary(x, skip=5)
    with pytest.raises(ValueError, match="at least 4"):
        DG.summary([r for r in x[:4]], skip=1)
    with pytest.raises(ValueError, match="floating point"):
        DG.summary(torch.zeros(8, 2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="floating point"):
        DG.ess(torch.zeros(8, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\[S, C, D\]"):
        DG.summary(torch.zeros(8))
    with pytest.raises(ValueError, match="cannot hold one coordinate"):
        DG.summary(x, workspace_bytes=64)


def test_module_is_exported():
    import hamiltorch_amd
    assert hamiltorch_amd.diagnostics is DG
    for name in ("summary", "ess", "rhat", "ess_min", "rhat_max", "plan", "LAG_BLOCK", "SEGMENT_ROWS"):
        assert hasattr(DG, name), name


# ---- the built kernels --------------------------------------------------------------------------------------------------------------
def test_no_scratch_and_four_waves_in_the_diagnostics_kernels(tmp_path):
    """the gfx950 code objects of csrc/diagnostics.hip: no kernel spills or uses scratch, and the lag kernel's registers leave four
    waves per SIMD (at most 128 of the 512 per lane)."""
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
            if name and "diag_" in name.group(1):
                g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))      # noqa: E731
                found[name.group(1)] = (g("vgpr_count") + int(re.match(r"\s*(\d+)", blk).group(1)), g("private_segment_fixed_size"), g("vgpr_spill_count"))
    for part in ("diag_moments_kernelIf", "diag_moments_kernelId", "diag_combine_kernelIf", "diag_combine_kernelId", "diag_lags_kernelIfLi%d" % DG.LAG_BLOCK,
                 "diag_lags_kernelIdLi%d" % DG.LAG_BLOCK, "diag_lag_reduce_kernel", "diag_finish_kernel"):
        hits = [k for k in found if part in k]
        assert len(hits) == 1, (part, sorted(found))
        regs, scratch, spills = found[hits[0]]
        assert scratch == 0 and spills == 0, (hits[0], found[hits[0]])
        if "diag_lags_kernel" in part:
            assert regs <= 128, (hits[0], regs)
