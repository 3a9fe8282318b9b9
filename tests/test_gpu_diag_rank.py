"""GPU: hamiltorch_amd.diagnostics.rank_summary (csrc/diagnostics_rank.hip, then the stages of csrc/diagnostics.hip) against scipy's
rankdata / ndtri, numpy's sort / quantile and the numpy restatement of tests/diag_cases.py, on every coordinate of every case of
tests/diag_rank_cases.py (the table's own soundness: tests/test_diag_rank_cases_cpu.py).

Tolerances: the ranks are integers or half-integers and (r - 3/8) / (N + 1/4) is one fp64 subtraction and one division on both sides, so
z differs from scipy's only by the two Phi^-1 routines (AS 241 PPND16 against cephes: 9e-16 relative on the host build, see the CPU
file); the indicators are exact.  From there on the kernels and the reference compute the same fp64 quantities with differently
ordered sums, and no pair sum of a Geyer walk of a derived series is within 1e-6 of zero, so the truncation point cannot move: every
ESS and R-hat at 1e-9 relative, as in tests/test_gpu_diagnostics.py.  The quantiles are two order statistics and numpy's lerp: 1e-12
relative, with an absolute term of 1e-12 standard deviations for quantiles near zero."""
import numpy as np
import pytest
import torch

import diag_cases as T0
import diag_rank_cases as R
import hmc_oracle as O
import hamiltorch_amd as ht
from hamiltorch_amd import _abi
from hamiltorch_amd import diagnostics as DG
from hamiltorch_amd.samplelist import as_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("ess_bulk", "ess_tail", "rhat", "rhat_bulk", "rhat_folded", "q05", "median", "q95")
STATS = FIELDS[:5]


def _np(t):
    return t.cpu().numpy()


def _close(got, ref, rtol, what, atol=None):
    """NaN exactly where the reference has NaN, inf where it has inf (R-hat of tied ranks with no within-chain spread); elsewhere
    |got - ref| <= rtol |ref| (+ atol)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, np.flatnonzero(np.isnan(got) != np.isnan(ref)))
    assert np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)]) and np.array_equal(np.isinf(got), np.isinf(ref)), what
    ok = np.isfinite(ref)
    if not ok.any():
        return
    bound = rtol * np.abs(ref[ok]) + (0.0 if atol is None else np.asarray(atol, dtype=np.float64)[ok])
    err = np.abs(got[ok] - ref[ok])
    print("%s: max relative difference %.3g" % (what, (err / np.maximum(np.abs(ref[ok]), 1e-300)).max()))
    assert np.all(err <= bound), (what, int(np.flatnonzero(ok)[(err - bound).argmax()]), got[ok][(err - bound).argmax()], ref[ok][(err - bound).argmax()])


def _check(s, ref, what=""):
    for f in STATS:
        _close(_np(getattr(s, f)), getattr(ref, f), 1e-9, what + f)
    for f in ("q05", "median", "q95"):
        _close(_np(getattr(s, f)), getattr(ref, f), 1e-12, what + f, atol=1e-12 * np.nan_to_num(ref.sd))


def _same_bits(a, b):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype == torch.float64 and x.shape == y.shape, f
        assert torch.equal(x.view(torch.int64), y.view(torch.int64)), f


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_parity_on_every_coordinate(case):
    x = torch.from_numpy(R.samples(case)).to(DEV)
    s = DG.rank_summary(x)
    assert s.route == "diag_rank_scatter_kernel<uint%d>" % (32 if case.dtype == np.float32 else 64)
    for f in FIELDS:
        t = getattr(s, f)
        assert t.shape == (case.D,) and t.device.type == "cuda" and t.dtype == torch.float64, f
    assert (s.n_draws, s.n_chains) == (case.S, case.C)
    ref = R.referenced(case)
    _check(s, ref)
    both = np.minimum(ref.ess_bulk, ref.ess_tail)
    if np.isnan(both).any():
        assert np.isnan(s.min_ess())
    else:
        assert abs(s.min_ess() - both.min()) <= 1e-9 * both.min()
    top = np.nanmax(ref.rhat)
    assert s.max_rhat() == top or abs(s.max_rhat() - top) <= 1e-9 * top
    if case.variant == "d":                                     # the degenerate coordinates, and their neighbours untouched (above)
        for f in FIELDS:
            v = _np(getattr(s, f))
            assert np.isnan(v[R.WITH_NAN]) and np.isnan(v[R.WITH_INF]), f
            assert np.isnan(v[R.CONSTANT]) or (f in ("q05", "median", "q95") and v[R.CONSTANT] == 2.5), f
            assert not np.isnan(v[[0, 2, 4, 6]]).any(), f


def test_both_zeros_tie():
    """-0.0 and +0.0 get one rank: flipping the sign of every zero changes no bit, and the normal scores are scipy's (which ties them)."""
    case = next(c for c in R.CASES if c.variant == "c" and c.dtype == np.float32)
    x = R.samples(case)
    zeros = x == 0
    assert np.signbit(x[zeros]).any() and not np.signbit(x[zeros]).all()
    y = x.copy()
    y[zeros] = -y[zeros]
    a, b = DG.rank_summary(torch.from_numpy(x).to(DEV)), DG.rank_summary(torch.from_numpy(y).to(DEV))
    _same_bits(a, b)
    w = np.where(zeros, np.float32(0.0), x)
    _same_bits(a, DG.rank_summary(torch.from_numpy(w).to(DEV)))


def test_the_derived_series_are_scipy_s():
    """the ABI stage by itself: z, I05, I95, zf of a tied and a float64 case, element by element."""
    lib = _abi.load()
    for case in (next(c for c in R.CASES if c.variant == "b" and c.D == 130 and c.dtype == np.float32), next(c for c in R.CASES if c.variant == "e" and c.C > 1)):
        xh = R.samples(case)
        x = torch.from_numpy(xh).to(DEV)
        S, C, D = x.shape
        z, zf = (torch.empty(S, C, D, dtype=torch.float64, device=DEV) for _ in range(2))
        i05, i95 = (torch.empty(S, C, D, dtype=torch.float32, device=DEV) for _ in range(2))
        q05, med, q95, centre = (torch.empty(D, dtype=torch.float64, device=DEV) for _ in range(4))
        bad = torch.full((D,), 7, dtype=torch.int32, device=DEV)
        nb = lib.hta_diag_rank_workspace_bytes(S, C, D, 8)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        suf = "f32" if case.dtype == np.float32 else "f64"
        p = lambda t: t.data_ptr()                                   # noqa: E731
        st = torch.cuda.current_stream().cuda_stream
        assert getattr(lib, "hta_diag_rank_" + suf)(p(x), C * D, D, S, C, D, p(z), p(i05), p(i95), p(q05), p(med), p(q95), p(centre), p(bad), p(ws), nb, st) == 0
        assert getattr(lib, "hta_diag_rank_folded_" + suf)(p(x), C * D, D, S, C, D, p(centre), p(zf), p(bad), p(ws), nb, st) == 0
        ref = R.referenced(case)
        assert int(bad.abs().sum()) == 0
        assert np.array_equal(_np(i05), ref.i05.astype(np.float32)) and np.array_equal(_np(i95), ref.i95.astype(np.float32))
        for got, want, what in ((z, ref.z, "z"), (zf, ref.zf, "zf")):
            err = np.abs(_np(got) - want) / np.maximum(np.abs(want), 1e-300)
            print("%s: max relative difference to ndtri %.3g" % (what, err.max()))
            assert err.max() <= 1e-14, what


@pytest.fixture(scope="module")
def wide():
    """[259, 3, 130] float32 with one leading row to skip, on the device (N = 774 after the skip; ties in the first coordinates)."""
    x = T0.generate(259, 3, 130, np.float32, 78)
    x[:, :, :5] = np.round(x[:, :, :5] * 2) / 2
    return torch.from_numpy(x).to(DEV)


def test_strided_views_give_the_bits_of_a_contiguous_copy(wide):
    k = 67
    view = wide[1:, :, :k]
    assert not view.is_contiguous()
    b = DG.rank_summary(view.contiguous())
    _same_bits(DG.rank_summary(view), b)
    _same_bits(DG.rank_summary(wide[:, :, :k], skip=1), b)
    _same_bits(DG.rank_summary(list(wide[:, :, :k].contiguous().unbind(0)), skip=1), b)
    one = DG.rank_summary(wide[1:, 1, :k])                      # [S, D]: one chain
    _same_bits(one, DG.rank_summary(wide[1:, 1:2, :k].contiguous()))
    assert one.n_chains == 1 and b.n_chains == 3 and b.n_draws == 258
    _check(one, R.reference(_np(wide[1:, 1:2, :k])), "one chain ")


def test_chunking_does_not_change_a_bit(wide):
    S, C, D = wide.shape
    cap = 50 * DG.rank_bytes_for(S, C, 1, DG.plan(S, C, D).lags_per_launch)
    assert len(DG.rank_plan(S, C, D, 4, cap).chunks) >= 3 and len(DG.rank_plan(S, C, D).chunks) == 1
    _same_bits(DG.rank_summary(wide, workspace_bytes=cap), DG.rank_summary(wide))


def test_two_calls_agree_bit_for_bit():
    case = next(c for c in R.CASES if c.variant == "b" and c.D == 130 and c.dtype == np.float32)
    x = torch.from_numpy(R.samples(case)).to(DEV)
    _same_bits(DG.rank_summary(x), DG.rank_summary(x))


def test_summary_is_not_disturbed():
    """summary() on the same input before and after a rank_summary() call: equal bits (the shared scratch is not corrupted)."""
    case = next(c for c in R.CASES if c.S == 257 and c.dtype == np.float32)
    x = torch.from_numpy(R.samples(case)).to(DEV)
    before = DG.summary(x)
    DG.rank_summary(x)
    after = DG.summary(x)
    for f in ("mean", "sd", "ess_bulk", "rhat", "tau", "lags_used", "truncated"):
        assert torch.equal(getattr(before, f), getattr(after, f)), f


def test_max_lag_is_honoured():
    case = next(c for c in R.CASES if c.S == 257 and c.dtype == np.float64)
    xh = R.samples(case)
    x = torch.from_numpy(xh).to(DEV)
    cut, full = R.reference(xh, max_lag=DG.LAG_BLOCK), R.referenced(case)
    assert np.nanmin(cut.small) >= 1e-6 and not np.allclose(cut.ess_bulk, full.ess_bulk, rtol=1e-6)
    s = DG.rank_summary(x, max_lag=DG.LAG_BLOCK)
    _check(s, cut, "max_lag ")
    _close(_np(DG.ess_tail(x, max_lag=DG.LAG_BLOCK)), cut.ess_tail, 1e-9, "ess_tail at max_lag")
    _close(_np(DG.ess_tail(x)), full.ess_tail, 1e-9, "ess_tail")
    assert torch.equal(DG.rhat_rank(x), DG.rank_summary(x).rhat)


def test_end_to_end_on_what_sample_returns():
    sigma = torch.tensor([[1.0, 0.6, 0.2], [0.6, 2.0, 0.5], [0.2, 0.5, 0.5]], device=DEV)
    C, N = 64, 200
    tgt = ht.GaussianTarget(torch.zeros(3, device=DEV), covariance=sigma)
    theta0 = 0.1 * torch.from_numpy(O.philox_normals(11, np.arange(C), 0, 3, O.PURPOSE_INIT)).to(DEV)
    out = ht.sample(tgt, theta0, num_samples=N, num_steps_per_sample=5, step_size=0.3, seed=11, verbose=False)
    assert isinstance(out, list) and len(out) == N
    s = DG.rank_summary(out, skip=1)
    assert s.route == "diag_rank_scatter_kernel<uint32>" and s.n_draws == N - 1 and s.n_chains == C
    rows = as_tensor(out)[1:].cpu()
    ref = R.reference(rows.numpy())
    assert np.nanmin(ref.small) >= 1e-6
    _check(s, ref, "sample() ")
    assert np.all(_np(s.rhat) < 1.05) and np.all(_np(s.ess_bulk) > 100) and np.all(_np(s.ess_tail) > 100)
    # a CPU tensor is staged and the results come back on the CPU
    h = DG.rank_summary(rows)
    for f in FIELDS:
        assert getattr(h, f).device.type == "cpu", f
        assert torch.equal(getattr(h, f).view(torch.int64), getattr(s, f).cpu().view(torch.int64)), f
    # half precision goes through float32
    _same_bits(DG.rank_summary(rows.to(torch.bfloat16).to(DEV)), DG.rank_summary(rows.to(torch.bfloat16).to(torch.float32).to(DEV)))


def test_bad_arguments_are_refused_before_any_launch():
    lib = _abi.load()
    x = torch.zeros(8, 2, 3, device=DEV)
    out = torch.empty(8 * 2 * 3, dtype=torch.float64, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    p = lambda t: t.data_ptr()                                   # noqa: E731
    rank = lambda ss, sc, S, C, D, nb: lib.hta_diag_rank_f32(p(x), ss, sc, S, C, D, p(out), p(out), p(out), p(out), p(out), p(out), p(out), p(out), p(ws), nb, None)  # noqa: E731
    assert rank(6, 3, 3, 2, 3, ws.numel()) == -1 and b"bad shape" in lib.hta_last_error()
    assert rank(6, 2, 8, 2, 3, ws.numel()) == -1 and b"bad strides" in lib.hta_last_error()
    assert rank(6, 3, 8, 2, 3, 64) == -1 and b"workspace" in lib.hta_last_error()
    assert rank(1 << 15, 1, 1 << 16, 1 << 15, 1, ws.numel()) == -1 and b"bad shape" in lib.hta_last_error()       # S C = 2^31: shape arithmetic alone
    assert lib.hta_diag_rank_folded_f32(p(x), 6, 3, 8, 2, 3, p(out), p(out), p(out), p(ws), 64, None) == -1 and b"workspace" in lib.hta_last_error()
    with pytest.raises(ValueError, match="2\\^31"):
        DG.rank_summary(torch.zeros(1, device=DEV).expand(1 << 16, 1 << 15, 1))
