"""CPU: the cases of tests/moments_cases.py - the band the running-moments kernels are held to is what the float64 restatement
itself loses against np.longdouble, measured here; the restatement's merge / stack / NaN rules; the library's error channel and
the code objects of csrc/moments.hip.  The kernels themselves: tests/test_gpu_moments.py."""
import ctypes

import numpy as np
import pytest

import moments_cases as cases
from hamiltorch_amd import diagnostics as DG


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_the_band_is_the_measured_error_of_the_restatement(case):
    """per quantity: what the restatement loses against longdouble is not above its record in MEASURED and (where the record is
    above the floor) not below half of it - the band is neither exceeded by its own reference nor padded."""
    got = cases.measure(case)
    print(case.name, got)
    rec, band = cases.MEASURED[case.name], cases.band(case)
    assert set(rec) == set(cases.QUANTITIES)
    for k in cases.QUANTITIES:
        assert got[k] <= rec[k], (k, got[k], rec[k])
        if rec[k] > cases.FLOOR:
            assert got[k] >= 0.5 * rec[k], (k, got[k], rec[k])
        assert band[k] == max(4 * rec[k], 1e-15)


def test_a_sum_of_squares_would_not_do():
    """the offset case (mean 1e6, sd 1, 1000 rows): M2 as sum x^2 - (sum x)^2 / n in float64 is 1e5 bands away from the
    longdouble value, Welford's recurrence is inside its record."""
    case = cases.BY_NAME["offset-f64"]
    x = np.asarray(cases.samples(case), dtype=np.float64)
    ref = cases.exact(x)["chain_m2"]
    naive = (x * x).sum(axis=0) - x.sum(axis=0) ** 2 / x.shape[0]
    err = float(np.abs(naive - ref).max() / np.abs(ref).max())
    print("sum of squares: relative error of M2 %.3g; Welford's record %.3g" % (err, cases.MEASURED[case.name]["chain_m2"]))
    assert err > 1e5 * cases.band(case)["chain_m2"]


def test_the_restatement_merges_and_stacks():
    """merge of two states = one state fed both (inside the band); stack of the halves gives ess.py's split R-hat."""
    import torch
    from hamiltorch_amd import ess as E
    case = cases.BY_NAME["S33-C64-D130-f64"]
    x = cases.samples(case)
    whole = cases.restate(x, (33,))
    a, b = cases.State().update(x[:13]), cases.State().update(x[13:])
    e = cases.errors(a.merge(b).finish(), whole, x)
    assert all(e[k] <= cases.band(case)[k] for k in cases.QUANTITIES), e
    x = x[:32]
    halves = cases.State.stack([cases.State().update(x[:16]), cases.State().update(x[16:])]).finish()
    want = np.array([E.rhat_split(torch.from_numpy(x[:, :, d].copy())) for d in range(case.D)])
    np.testing.assert_allclose(halves["rhat"], want, rtol=1e-12)


def test_one_nan_draw_poisons_its_own_series_only():
    case = cases.BY_NAME["nan-f64"]
    x = cases.samples(case)
    _, c, d = cases.NAN_AT
    for chunks in cases.chunkings(case.S):
        r = cases.restate(x, chunks)
        bad = np.zeros((case.C, case.D), bool)
        bad[c, d] = True
        assert np.array_equal(np.isnan(r["chain_mean"]), bad) and np.array_equal(np.isnan(r["chain_m2"]), bad)
        for k in ("mean", "var_within", "var_between", "var_total", "rhat", "inv_mass"):
            assert np.array_equal(np.isnan(r[k]), np.arange(case.D) == d), k


def test_segment_rows_restated():
    """diagnostics.moments_segment_rows: 256 rows where C D fills the machine, halved down to 32 while the grid is small; the
    (600, 2, 3) case is cut into more than two segments; a block of the warm-up is one segment (no workspace, one launch)."""
    assert DG.moments_segment_rows(1000, 1024, 128) == 256
    assert DG.moments_segment_rows(600, 2, 3) == 32 and -(-600 // 32) > 2
    assert DG.moments_segment_rows(1000, 1024, 3) == 32
    assert DG.moments_segment_rows(9, 64, 4) == 32 and -(-9 // 32) == 1
    for S, C, D in ((200, 1024, 128), (1000, 1024, 3), (600, 2, 3), (9, 64, 4), (1, 1, 1)):
        R = DG.moments_segment_rows(S, C, D)
        nseg = -(-S // R)
        from hamiltorch_amd import _abi
        assert _abi.load().hta_moments_workspace_bytes(S, C, D) == (16 * nseg * C * D if nseg > 1 else 0)


def test_the_library_refuses_bad_arguments_without_a_device():
    """before any launch, and so also where there is no GPU: NULL pointers, a short workspace, bad shapes and strides."""
    from hamiltorch_amd import _abi
    lib = _abi.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 40
    assert lib.hta_moments_update_f32(None, 6, 3, 600, 2, 3, 0, p, p, big, None) == -1 and b"NULL" in lib.hta_last_error()
    assert lib.hta_moments_update_f64(p, 6, 3, 600, 2, 3, 0, None, p, big, None) == -1 and b"NULL" in lib.hta_last_error()
    need = lib.hta_moments_workspace_bytes(600, 2, 3)
    assert need > 0
    assert lib.hta_moments_update_f32(p, 6, 3, 600, 2, 3, 0, p, p, need - 8, None) == -1 and b"workspace" in lib.hta_last_error()
    assert lib.hta_moments_update_f32(p, 6, 3, 600, 2, 3, 0, p, None, need, None) == -1 and b"workspace" in lib.hta_last_error()
    assert lib.hta_moments_update_f32(p, 6, 3, 0, 2, 3, 0, p, p, big, None) == -1 and b"bad shape" in lib.hta_last_error()
    assert lib.hta_moments_update_f64(p, 6, 3, 5, 2, 0, 0, p, p, big, None) == -1 and b"bad shape" in lib.hta_last_error()
    assert lib.hta_moments_update_f64(p, 6, 3, 5, 1 << 31, 3, 0, p, p, big, None) == -1 and b"bad shape" in lib.hta_last_error()
    assert lib.hta_moments_update_f32(p, 6, 2, 5, 2, 3, 0, p, p, big, None) == -1 and b"bad strides" in lib.hta_last_error()
    assert lib.hta_moments_update_f32(p, 5, 3, 5, 2, 3, 0, p, p, big, None) == -1 and b"bad strides" in lib.hta_last_error()
    assert lib.hta_moments_update_f32(p, 6, 3, 5, 2, 3, -1, p, p, big, None) == -1 and b"n_prev" in lib.hta_last_error()
    assert lib.hta_moments_workspace_bytes(0, 2, 3) == -1 and lib.hta_moments_workspace_bytes(5, 2, -1) == -1
    fin = lambda C, D, n, st: lib.hta_moments_finish(C, D, n, st, p, p, p, p, p, 5.0, 1e-3, None, p, None)      # noqa: E731
    assert fin(2, 3, 10, None) == -1 and b"NULL" in lib.hta_last_error()
    assert fin(0, 3, 10, p) == -1 and b"bad shape" in lib.hta_last_error()
    assert fin(2, 3, 0, p) == -1 and b"draws" in lib.hta_last_error()
    assert lib.hta_moments_finish(2, 3, 10, p, p, p, p, p, p, -1.0, 1e-3, None, p, None) == -1 and b"regularisation" in lib.hta_last_error()


def test_running_moments_refuses_bad_input_without_a_device():
    import torch
    with pytest.raises(ValueError, match="both C and D"):
        DG.RunningMoments(3)
    with pytest.raises(ValueError, match="no draws"):
        DG.RunningMoments().result()
    with pytest.raises(ValueError, match="floating point"):
        DG.RunningMoments().update(torch.zeros(8, 2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"\[S, C, D\]"):
        DG.RunningMoments().update(torch.zeros(8))
    with pytest.raises(ValueError, match="skip"):
        DG.RunningMoments().update(torch.zeros(8, 2, 3), skip=-1)
    acc = DG.RunningMoments()
    assert acc.update(torch.zeros(3, 2, 3), skip=3) is acc and acc.n_draws == 0 and acc.n_chains is None     # nothing to add: no device needed
    with pytest.raises(ValueError, match="without a shape"):
        DG.RunningMoments.stack([DG.RunningMoments()])


def test_module_exports_the_moments_names():
    import hamiltorch_amd
    from hamiltorch_amd import _abi
    assert hamiltorch_amd.diagnostics is DG
    for name in ("RunningMoments", "MomentsResult", "moments_segment_rows"):
        assert hasattr(DG, name), name
    assert "hta_moments_update" in _abi.TYPED_SYMBOLS and {"hta_moments_workspace_bytes", "hta_moments_finish"} <= set(_abi.PLAIN_SYMBOLS)
    assert _abi.ABI_VERSION == 17


def test_no_scratch_and_no_spills_in_the_moments_kernels(tmp_path):
    """the gfx950 code objects of csrc/moments.hip: every instance of every kernel is there, none spills or uses scratch."""
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
            if name and "moments_" in name.group(1) and "diag_" not in name.group(1):
                g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))      # noqa: E731
                found[name.group(1)] = (g("vgpr_count"), g("private_segment_fixed_size"), g("vgpr_spill_count"), g("sgpr_spill_count"))
    print(found)
    for part, instances in (("moments_update_kernel", 2), ("moments_merge_kernel", 1), ("moments_finish_kernel", 1)):
        hits = [k for k in found if part in k]
        assert len(hits) == instances, (part, sorted(found))
        for k in hits:
            assert found[k][1:] == (0, 0, 0), (k, found[k])
