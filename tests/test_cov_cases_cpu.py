"""CPU: the cases of tests/cov_cases.py - the band the running-covariance kernels are held to is what the float64 restatement
itself loses against np.longdouble, measured here; the restatement's means and diagonal are the moments restatement's bits; its
NaN rule; the library's error channel; and the dense mode of adapt.Controller.  The kernels themselves: tests/test_gpu_cov.py."""
import ctypes

import numpy as np
import pytest

import cov_cases as cases
import moments_cases as MC
from hamiltorch_amd import adapt
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


def test_the_cases_reach_their_edges():
    shapes = {(c.S, c.C, c.D) for c in cases.CASES}
    assert {(1, 1, 1), (5, 3, 1), (7, 65, 3), (4, 1025, 2), (600, 2, 3), (9, 3, 17), (5, 3, 64), (3, 2, 256)} <= shapes
    assert -(-600 // DG.moments_segment_rows(600, 2, 3)) > 2
    assert 17 * 18 // 2 == 153 and 153 % 64 and 64 * 65 // 2 == 2080 and DG.COVARIANCE_MAX_D == 256
    for kind in ("offset", "constant", "nan"):
        assert any(c.kind == kind for c in cases.CASES)


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_means_and_diagonal_are_the_moments_restatement_bit_for_bit(case):
    """every chunking: the means, the diagonal co-moments and the diagonal outputs of the covariance restatement equal
    moments_cases.State's on the same feed, bit for bit (NaN where it has NaN); the matrices are exactly symmetric."""
    x = cases.samples(case)
    iu, ju = cases.pairs(case.D)
    for chunks in cases.chunkings(case.S):
        a, b, r0 = cases.State(), MC.State(), 0
        for k in chunks:
            a.update(x[r0:r0 + k])
            b.update(x[r0:r0 + k])
            r0 += k
        assert np.array_equal(a.mean, b.mean, equal_nan=True) and np.array_equal(a.q[:, iu == ju], b.m2, equal_nan=True)
        fa, fb = a.finish(), b.finish()
        assert np.array_equal(fa["mean"], fb["mean"], equal_nan=True) and np.array_equal(fa["rhat"], fb["rhat"], equal_nan=True)
        for k, k1 in (("cov_within", "var_within"), ("cov_total", "var_total"), ("inv_mass", "inv_mass")):
            assert np.array_equal(np.diag(fa[k]), fb[k1], equal_nan=True), k
            assert np.array_equal(fa[k], fa[k].T, equal_nan=True), k


def test_the_restatement_is_the_covariance():
    """against numpy.cov of the pooled draws and of each chain (1e-12), and merge of two states = one state fed both."""
    case = cases.BY_NAME["S9-C3-D17-f64"]
    x = cases.samples(case)
    r = cases.restate(x, (9,))
    np.testing.assert_allclose(r["cov_total"], np.cov(x.reshape(-1, case.D), rowvar=False), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(r["cov_within"], np.mean([np.cov(x[:, c], rowvar=False) for c in range(case.C)], axis=0), rtol=1e-11, atol=1e-12)
    N = 27.0
    np.testing.assert_allclose(r["inv_mass"], r["cov_total"] * (N / (N + 5.0)) + 1e-3 * (5.0 / (N + 5.0)) * np.eye(case.D), rtol=1e-14)
    merged = cases.State().update(x[:4]).merge(cases.State().update(x[4:])).finish()
    e = cases.errors(merged, r, x)
    assert all(e[k] <= cases.band(case)[k] for k in cases.QUANTITIES), e


def test_one_nan_draw_poisons_its_own_pairs_only():
    """NaN in mean[c][d] and in every co-moment of chain c that involves d - nowhere else; pooled: row and column d."""
    case = cases.BY_NAME["nan-f64"]
    x = cases.samples(case)
    _, c, d = cases.NAN_AT
    iu, ju = cases.pairs(case.D)
    for chunks in cases.chunkings(case.S):
        r = cases.restate(x, chunks)
        bad_m = np.zeros((case.C, case.D), bool)
        bad_m[c, d] = True
        bad_q = np.zeros((case.C, iu.size), bool)
        bad_q[c] = (iu == d) | (ju == d)
        assert np.array_equal(np.isnan(r["chain_mean"]), bad_m) and np.array_equal(np.isnan(r["chain_q"]), bad_q)
        line = np.arange(case.D) == d
        for k in ("mean", "rhat"):
            assert np.array_equal(np.isnan(r[k]), line), k
        for k in ("cov_within", "cov_total", "inv_mass"):
            assert np.array_equal(np.isnan(r[k]), line[:, None] | line[None, :]), k


def test_the_library_refuses_bad_arguments_without_a_device():
    """before any launch, and so also where there is no GPU: NULL pointers, alignment, overlapping strides, a short workspace,
    n_prev, D over the limit and the regularisation values."""
    from hamiltorch_amd import _abi
    lib = _abi.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    big = 1 << 40
    assert lib.hta_cov_update_f32(None, 6, 3, 600, 2, 3, 0, p, p, big, None) == -1 and b"NULL" in lib.hta_last_error()
    assert lib.hta_cov_update_f64(p, 6, 3, 600, 2, 3, 0, None, p, big, None) == -1 and b"NULL" in lib.hta_last_error()
    assert lib.hta_cov_update_f64(p, 6, 3, 5, 2, 3, 0, odd, p, big, None) == -1 and b"aligned" in lib.hta_last_error()
    need = lib.hta_cov_workspace_bytes(600, 2, 3)
    nseg = -(-600 // DG.moments_segment_rows(600, 2, 3))
    assert need == 8 * nseg * 2 * (3 + 6) and lib.hta_cov_workspace_bytes(9, 64, 6) == 0
    assert lib.hta_cov_state_bytes(1024, 256) == 8 * 1024 * (256 + 32896) and lib.hta_cov_state_bytes(2, 3) == 8 * 2 * 9
    assert lib.hta_cov_update_f32(p, 6, 3, 600, 2, 3, 0, p, p, need - 8, None) == -1 and b"workspace" in lib.hta_last_error()
    assert lib.hta_cov_update_f32(p, 6, 3, 600, 2, 3, 0, p, None, need, None) == -1 and b"workspace" in lib.hta_last_error()
    assert lib.hta_cov_update_f32(p, 6, 3, 600, 2, 3, 0, p, odd, big, None) == -1 and b"workspace" in lib.hta_last_error()
    assert lib.hta_cov_update_f32(p, 6, 3, 0, 2, 3, 0, p, p, big, None) == -1 and b"bad shape" in lib.hta_last_error()
    assert lib.hta_cov_update_f64(p, 6, 3, 5, 2, 0, 0, p, p, big, None) == -1 and b"bad shape" in lib.hta_last_error()
    assert lib.hta_cov_update_f64(p, 6, 3, 5, 1 << 31, 3, 0, p, p, big, None) == -1 and b"bad shape" in lib.hta_last_error()
    assert lib.hta_cov_update_f32(p, 600, 257, 5, 2, 257, 0, p, p, big, None) == -1 and b"limit of 256" in lib.hta_last_error()
    assert lib.hta_cov_update_f32(p, 6, 2, 5, 2, 3, 0, p, p, big, None) == -1 and b"bad strides" in lib.hta_last_error()
    assert lib.hta_cov_update_f32(p, 5, 3, 5, 2, 3, 0, p, p, big, None) == -1 and b"bad strides" in lib.hta_last_error()
    assert lib.hta_cov_update_f32(p, 6, 3, 5, 2, 3, -1, p, p, big, None) == -1 and b"n_prev" in lib.hta_last_error()
    assert lib.hta_cov_workspace_bytes(0, 2, 3) == -1 and lib.hta_cov_workspace_bytes(5, 2, 257) == -1
    assert lib.hta_cov_state_bytes(2, 257) == -1 and lib.hta_cov_state_bytes(0, 3) == -1
    fin = lambda C, D, n, st: lib.hta_cov_finish(C, D, n, st, p, p, p, p, 5.0, 1e-3, None, p, None)      # noqa: E731
    assert fin(2, 3, 10, None) == -1 and b"NULL" in lib.hta_last_error()
    assert fin(2, 3, 10, odd) == -1 and b"aligned" in lib.hta_last_error()
    assert fin(0, 3, 10, p) == -1 and b"bad shape" in lib.hta_last_error()
    assert fin(2, 257, 10, p) == -1 and b"limit of 256" in lib.hta_last_error()
    assert fin(2, 3, 0, p) == -1 and b"draws" in lib.hta_last_error()
    assert lib.hta_cov_finish(2, 3, 10, p, p, p, p, p, -1.0, 1e-3, None, p, None) == -1 and b"regularisation" in lib.hta_last_error()
    assert lib.hta_cov_finish(2, 3, 10, p, p, p, p, p, 5.0, -1e-3, p, None, None) == -1 and b"regularisation" in lib.hta_last_error()


def test_running_covariance_refuses_bad_input_without_a_device():
    import torch
    with pytest.raises(ValueError, match="both C and D"):
        DG.RunningCovariance(3)
    with pytest.raises(ValueError, match="limit of 256"):
        DG.RunningCovariance(2, 257, "cuda")
    with pytest.raises(ValueError, match="limit of 256"):
        DG.RunningCovariance().update(torch.zeros(4, 2, 257))
    with pytest.raises(ValueError, match="no draws"):
        DG.RunningCovariance().result()
    with pytest.raises(ValueError, match="floating point"):
        DG.RunningCovariance().update(torch.zeros(8, 2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"\[S, C, D\]"):
        DG.RunningCovariance().update(torch.zeros(8))
    with pytest.raises(ValueError, match="skip"):
        DG.RunningCovariance().update(torch.zeros(8, 2, 3), skip=-1)
    acc = DG.RunningCovariance()
    assert acc.update(torch.zeros(3, 2, 3), skip=3) is acc and acc.n_draws == 0 and acc.n_chains is None     # nothing to add: no device needed
    with pytest.raises(ValueError, match="without a shape"):
        DG.RunningCovariance.stack([DG.RunningCovariance()])


def test_module_exports_the_covariance_names():
    import hamiltorch_amd
    from hamiltorch_amd import _abi
    assert hamiltorch_amd.diagnostics is DG
    for name in ("RunningCovariance", "CovarianceResult", "COVARIANCE_MAX_D"):
        assert hasattr(DG, name), name
    assert "hta_cov_update" in _abi.TYPED_SYMBOLS and {"hta_cov_workspace_bytes", "hta_cov_state_bytes", "hta_cov_finish"} <= set(_abi.PLAIN_SYMBOLS)
    assert _abi.ABI_VERSION == 17 and _abi.load().hta_abi_version() == 17


def _windows(ctl, masses):
    seen = []
    for m in masses:
        ctl.next_block()
        ctl.observe_block(0.8)
        ctl.observe_window(m)
        seen.append(ctl.inv_mass)
    return seen


@pytest.mark.parametrize("form", ["numpy", "torch"])
def test_controller_dense_refuses_bad_matrices(form):
    """mass="dense" on the host: the first refusal keeps the identity, a later one the previous matrix; a non-finite, an
    indefinite and a singular matrix are refused; the history records `accepted`."""
    import torch
    conv = (lambda a: np.array(a, dtype=np.float32)) if form == "numpy" else (lambda a: torch.tensor(a, dtype=torch.float32))
    good = conv([[2.0, 0.5], [0.5, 1.0]])
    masses = [conv([[1.0, float("nan")], [float("nan"), 1.0]]), good, conv([[1.0, 2.0], [2.0, 1.0]]), conv([[1.0, 1.0], [1.0, 1.0]]),
              conv([[float("inf"), 0.0], [0.0, 1.0]])]
    ctl = adapt.Controller(0.1, block=1, windows=(1,) * 5, settle=0, mass="dense")
    assert ctl.mass == "dense"
    seen = _windows(ctl, masses)
    assert np.array_equal(np.asarray(seen[0]), np.eye(2, dtype=np.float32)) and np.asarray(seen[0]).dtype == np.float32
    assert type(seen[0]) is type(good)
    assert all(s is good for s in seen[1:])
    wins = [h for h in ctl.history if h["kind"] == "window"]
    assert [h["accepted"] for h in wins] == [False, True, False, False, False] and all(type(h["accepted"]) is bool for h in wins)


def test_controller_mass_argument():
    with pytest.raises(ValueError, match="banana"):
        adapt.Controller(0.1, mass="banana")
    assert adapt.Controller(0.1).mass == "diag" and adapt.Controller(0.1, 10, (5,), 5, 0.8, True, 5, 1e-3).mass == "diag"
    ctl = adapt.Controller(0.1, block=1, windows=(1, 1), settle=0)                     # the diagonal mode: as before
    seen = _windows(ctl, [np.array([1.0, 2.0]), np.array([1.0, -2.0])])
    assert np.array_equal(seen[0], [1.0, 2.0]) and seen[1] is seen[0]
    ctl = adapt.Controller(0.1, block=1, windows=(1,), settle=0)
    ctl.next_block()
    ctl.observe_block(0.8)
    with pytest.raises(ValueError, match=r"\(D,\)"):
        ctl.observe_window(np.eye(2))
    dense = adapt.Controller(0.1, block=1, windows=(1,), settle=0, mass="dense")
    dense.next_block()
    dense.observe_block(0.8)
    with pytest.raises(ValueError, match=r"\(D, D\)"):
        dense.observe_window(np.ones(2))


def test_warmup_dense_refuses_other_samplers_and_large_d():
    import torch
    import hamiltorch_amd as ht
    f = lambda th: -(th * th).sum()                                          # noqa: E731
    with pytest.raises(ValueError, match="RMHMC"):
        ht.warmup(f, torch.zeros(8, 3), mass="dense", sampler=ht.Sampler.RMHMC)
    with pytest.raises(ValueError, match="HMC_NUTS"):
        ht.warmup(f, torch.zeros(8, 3), mass="dense", sampler=ht.Sampler.HMC_NUTS)
    with pytest.raises(ValueError, match="D <= 256"):
        ht.warmup(f, torch.zeros(8, 257), mass="dense")
    with pytest.raises(ValueError, match="banana"):
        ht.warmup(f, torch.zeros(8, 3), mass="banana")
