"""GPU: hamiltorch_amd.diagnostics (csrc/diagnostics.hip) against the oracle's ess_bulk, ess.py's rhat_split and the numpy
restatement of tests/diag_cases.py, on every coordinate of every case of its table (the table's own soundness: tests/test_diag_cases_cpu.py).

Tolerances: the kernels and the references compute the same fp64 quantities with differently ordered sums; direct summation and the
FFT form agree to 2.3e-13 on these cases, and no pair sum of a Geyer walk is within 1e-6 of zero, so the truncation point cannot move:
ess / tau / rhat at 1e-9 relative, mean and sd at 1e-12 relative, lags_used exactly."""
import numpy as np
import pytest
import torch

import diag_cases as T
import hmc_oracle as O
import hamiltorch_amd as ht
from hamiltorch_amd import _abi
from hamiltorch_amd import diagnostics as DG
from hamiltorch_amd import ess as E
from hamiltorch_amd.samplelist import as_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("mean", "sd", "ess_bulk", "rhat", "tau", "lags_used", "truncated")


def _np(t):
    return t.cpu().numpy()


def _close(got, ref, rtol, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref) / np.abs(ref)
    print("%s: max relative difference %.3g" % (what, err.max()))
    assert np.all(err <= rtol), (what, int(err.argmax()), got[err.argmax()], ref[err.argmax()])


def _same_bits(a, b):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape, f
        assert torch.equal(x, y) if not x.is_floating_point() else torch.equal(x.view(torch.int64), y.view(torch.int64)), f


@pytest.mark.parametrize("case", T.CASES, ids=T.IDS)
def test_parity_on_every_coordinate(case):
    x = torch.from_numpy(T.samples(case)).to(DEV)
    s = DG.summary(x)
    assert "diag_lags_kernel<%s,%d>" % ("float" if case.dtype == np.float32 else "double", DG.LAG_BLOCK) == _abi.last_route()
    ref, r = T.reference(case), T.restated(case)
    for f in FIELDS:
        t = getattr(s, f)
        assert t.shape == (case.D,) and t.device.type == "cuda", f
    assert (s.n_draws, s.n_chains) == (case.S, case.C)
    _close(_np(s.ess_bulk), ref.ess, 1e-9, "ess_bulk")
    _close(_np(s.tau), case.S * case.C / ref.ess, 1e-9, "tau")
    _close(_np(s.rhat), ref.rhat, 1e-9, "rhat")
    _close(_np(s.mean), r.mean, 1e-12, "mean")
    _close(_np(s.sd), r.sd, 1e-12, "sd")
    assert np.array_equal(_np(s.lags_used), r.lags)
    assert _np(s.truncated).all()
    assert abs(s.min_ess() - ref.ess.min()) <= 1e-9 * ref.ess.min() and abs(s.max_rhat() - ref.rhat.max()) <= 1e-9 * ref.rhat.max()


def test_more_chains_than_chain_groups():
    """beyond the table: C > CHAIN_GROUPS, where a lane of the lag kernel walks several chains."""
    C = DG.CHAIN_GROUPS + 6
    x = T.generate(2 * T.B + 1, C, 3, np.float32, 31)
    s = DG.summary(torch.from_numpy(x).to(DEV))
    r = T.restate(x)
    assert r.small.min() >= 1e-6
    _close(_np(s.ess_bulk), [O.ess_bulk(x[:, :, d]) for d in range(3)], 1e-9, "ess_bulk")
    _close(_np(s.tau), r.tau, 1e-9, "tau")
    _close(_np(s.rhat), r.rhat, 1e-9, "rhat")
    _close(_np(s.mean), r.mean, 1e-12, "mean")
    _close(_np(s.sd), r.sd, 1e-12, "sd")
    assert np.array_equal(_np(s.lags_used), r.lags)


@pytest.fixture(scope="module")
def wide():
    """[R + 2, 3, 130] float32 with one leading row to skip, on the device."""
    return torch.from_numpy(T.generate(T.R + 2, 3, 130, np.float32, 77)).to(DEV)


def test_strided_views_give_the_bits_of_a_contiguous_copy(wide):
    k = 67
    view = wide[1:, :, :k]
    assert not view.is_contiguous()
    a = DG.summary(view)
    b = DG.summary(view.contiguous())
    c = DG.summary(wide[:, :, :k], skip=1)
    d = DG.summary(list(wide[:, :, :k].contiguous().unbind(0)), skip=1)
    _same_bits(a, b)
    _same_bits(c, b)
    _same_bits(d, b)
    one = DG.summary(wide[1:, 1, :k])                         # [S, D]: one chain
    _same_bits(one, DG.summary(wide[1:, 1:2, :k].contiguous()))
    assert one.n_chains == 1


def test_chunking_does_not_change_a_bit(wide):
    S, C, D = wide.shape
    cap = 50 * DG.workspace_bytes_for(S, C, 1, DG.plan(S, C, D).lags_per_launch)
    assert len(DG.plan(S, C, D, 4, cap).chunks) >= 3 and len(DG.plan(S, C, D).chunks) == 1
    _same_bits(DG.summary(wide, workspace_bytes=cap), DG.summary(wide))


def test_two_calls_agree_bit_for_bit():
    case = T.CASES[T.IDS.index("S%d-C70-D67-f32" % T.R)]
    x = torch.from_numpy(T.samples(case)).to(DEV)
    a, b = DG.summary(x), DG.summary(x)
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f


def test_degenerate_columns():
    """a constant coordinate and one with a NaN in one row: NaN for those two after the first lag round, the others untouched."""
    x = T.generate(2 * T.B + 1, 3, 5, np.float32, 5)
    x[:, :, 1] = 2.5
    x[7, 2, 3] = np.nan
    s = DG.summary(torch.from_numpy(x).to(DEV))
    ok = [0, 2, 4]
    r = T.restate(x[:, :, ok])
    for d in (1, 3):
        assert np.isnan(float(s.ess_bulk[d])) and np.isnan(float(s.tau[d])) and int(s.lags_used[d]) <= DG.LAG_BLOCK
    assert np.isnan(float(s.rhat[3])) and np.isnan(float(s.mean[3])) and float(s.mean[1]) == 2.5 and float(s.sd[1]) == 0.0
    _close(_np(s.ess_bulk)[ok], [O.ess_bulk(x[:, :, d]) for d in ok], 1e-9, "ess_bulk")
    _close(_np(s.rhat)[ok], [E.rhat_split(torch.from_numpy(x[:, :, d])) for d in ok], 1e-9, "rhat")
    _close(_np(s.mean)[ok], r.mean, 1e-12, "mean")
    _close(_np(s.sd)[ok], r.sd, 1e-12, "sd")
    assert np.array_equal(_np(s.lags_used)[ok], r.lags)
    assert np.isnan(s.min_ess()) and abs(s.max_rhat() - np.nanmax(_np(s.rhat))) == 0.0
    # all coordinates degenerate: the call returns after the first round
    y = np.full((3 * T.B, 2, 2), 1.5, np.float64)
    s = DG.summary(torch.from_numpy(y).to(DEV))
    assert torch.isnan(s.ess_bulk).all() and int(s.lags_used.max()) == 0 and bool(s.truncated.all())


def test_max_lag_stops_a_walk_that_would_run_to_the_end():
    case, d = T.run_to_the_end_case()
    x = T.samples(case)
    s = DG.summary(torch.from_numpy(x).to(DEV), max_lag=DG.LAG_BLOCK)
    cut = T.restate(x, max_lag=DG.LAG_BLOCK)
    assert not cut.own[d] and not bool(s.truncated[d]) and int(s.lags_used[d]) == DG.LAG_BLOCK
    assert np.array_equal(_np(s.truncated), cut.own) and np.array_equal(_np(s.lags_used), cut.lags)
    _close(_np(s.tau), cut.tau, 1e-9, "tau at max_lag")
    _close(_np(DG.ess(torch.from_numpy(x).to(DEV), max_lag=DG.LAG_BLOCK)), cut.ess, 1e-9, "ess at max_lag")


def test_end_to_end_on_what_sample_returns():
    sigma = torch.tensor([[1.0, 0.6, 0.2], [0.6, 2.0, 0.5], [0.2, 0.5, 0.5]], device=DEV)
    C, N = 64, 200
    tgt = ht.GaussianTarget(torch.zeros(3, device=DEV), covariance=sigma)
    theta0 = 0.1 * torch.from_numpy(O.philox_normals(11, np.arange(C), 0, 3, O.PURPOSE_INIT)).to(DEV)
    out = ht.sample(tgt, theta0, num_samples=N, num_steps_per_sample=5, step_size=0.3, seed=11, verbose=False)
    assert isinstance(out, list) and len(out) == N
    s = DG.summary(out, skip=1)
    assert "diag_lags_kernel<float," in _abi.last_route()
    rows = as_tensor(out)[1:].cpu()
    e, r = E.ess_min(rows), E.rhat_max(rows)
    assert s.n_draws == N - 1 and s.n_chains == C
    assert abs(s.min_ess() - e) <= 1e-9 * e and abs(s.max_rhat() - r) <= 1e-9 * r
    assert abs(DG.ess_min(out, skip=1) - e) <= 1e-9 * e and abs(DG.rhat_max(out, skip=1) - r) <= 1e-9 * r
    assert torch.equal(DG.rhat(out, skip=1), s.rhat)
    # a CPU tensor is staged and the results come back on the CPU
    h = DG.summary(rows)
    for f in FIELDS:
        assert getattr(h, f).device.type == "cpu", f
        assert torch.equal(getattr(h, f), getattr(s, f).cpu()), f


def test_bad_arguments_are_refused_before_any_launch():
    lib = _abi.load()
    x = torch.zeros(8, 2, 3, device=DEV)
    out = torch.empty(3, dtype=torch.float64, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    p = lambda t: t.data_ptr()                                   # noqa: E731
    assert lib.hta_diag_moments_f32(p(x), 6, 3, 3, 2, 3, p(out), p(out), p(out), p(ws), ws.numel(), None) == -1 and b"bad shape" in lib.hta_last_error()
    assert lib.hta_diag_moments_f32(p(x), 6, 2, 8, 2, 3, p(out), p(out), p(out), p(ws), ws.numel(), None) == -1 and b"bad strides" in lib.hta_last_error()
    assert lib.hta_diag_moments_f32(p(x), 6, 3, 8, 2, 3, p(out), p(out), p(out), p(ws), 64, None) == -1 and b"workspace" in lib.hta_last_error()
    assert lib.hta_diag_lags_f32(p(x), 6, 3, 8, 2, 3, 8, 16, p(ws), ws.numel(), None) == -1 and b"bad lag range" in lib.hta_last_error()
