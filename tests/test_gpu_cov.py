"""GPU: diagnostics.RunningCovariance (csrc/covariance.hip) against the numpy restatement of tests/cov_cases.py on every case and
chunking, inside the band measured in tests/test_cov_cases_cpu.py (4 x what the restatement loses against longdouble, at least
1e-15); equal bits on strided views; merge, reset, stack; the NaN rule; and the bits it shares with RunningMoments."""
import numpy as np
import pytest
import torch

import cov_cases as cases
from hamiltorch_amd import _abi
from hamiltorch_amd import diagnostics as DG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MATRICES = ("cov_within", "cov_total", "inv_mass")


def quantities(acc):
    """A RunningCovariance's state and result as the restatement's dict of numpy arrays."""
    r = acc.result(reg_n=cases.REG_N, reg_floor=cases.REG_FLOOR, dtype=torch.float64)
    out = dict(chain_mean=acc.means, chain_q=acc.comoments, mean=r.mean, cov_within=r.cov_within, cov_total=r.cov_total, rhat=r.rhat, inv_mass=r.inv_mass)
    return {k: v.cpu().numpy() for k, v in out.items()}, r


def fed(x, chunks, form="tensor", cls=DG.RunningCovariance):
    """The accumulator of x[S, C, D] (a device tensor) fed `chunks` rows at a time."""
    acc, r0 = cls(), 0
    for k in chunks:
        part = x[r0:r0 + k]
        acc.update(list(part.unbind(0)) if form == "list" else part)
        r0 += k
    return acc


def inside(got, ref, case, x, what):
    e, band = cases.errors(got, ref, x), cases.band(case)
    print(what, {k: "%.2g" % v for k, v in e.items()})
    for k in cases.QUANTITIES:
        assert e[k] <= band[k], (what, k, e[k], band[k])
    for k in MATRICES:
        assert np.array_equal(got[k], got[k].T, equal_nan=True), (what, k, "not symmetric")


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_chunked_updates_equal_numpy(case):
    """every chunking of every case, as a tensor, as the list sample() returns and as a strided view (skip, a slice of chains
    of a larger buffer), against the restatement with the same chunking."""
    xn = cases.samples(case)
    x = torch.from_numpy(xn.copy()).to(DEV)
    big = torch.full((case.S + 2, case.C + 3, case.D + 1), 7.0, dtype=x.dtype, device=DEV)
    big[2:, 1:case.C + 1, :case.D] = x
    for chunks in cases.chunkings(case.S):
        ref = cases.restate(xn, chunks)
        acc = fed(x, chunks)
        assert _abi.last_route() == "cov_update_kernel<%s>" % ("float" if case.dtype == np.float32 else "double")
        got, r = quantities(acc)
        assert (acc.n_draws, acc.n_chains, acc.n_coordinates) == (case.S, case.C, case.D) == (r.n_draws, r.n_chains, r.mean.numel())
        assert r.mean.device.type == "cuda" and r.inv_mass.dtype == torch.float64 and r.inv_mass.shape == (case.D, case.D)
        inside(got, ref, case, xn, "%s %s" % (case.name, chunks))
        inside(quantities(fed(x, chunks, "list"))[0], ref, case, xn, "%s %s list" % (case.name, chunks))
    # the strided view: one update(skip=2) of the chain slice, = the restatement fed all rows at once
    view = big[:, 1:case.C + 1, :case.D]
    assert not view.is_contiguous()
    acc = DG.RunningCovariance(case.C, case.D, DEV).update(view, skip=2)
    inside(quantities(acc)[0], cases.restate(xn, (case.S,)), case, xn, "%s view" % case.name)
    r32 = acc.result(reg_n=cases.REG_N)
    assert r32.inv_mass.dtype == torch.float32 and acc.result().inv_mass is None
    got = quantities(acc)[0]
    np.testing.assert_array_equal(r32.inv_mass.cpu().numpy(), got["inv_mass"].astype(np.float32))        # the float32 output: the fp64 value, rounded once
    sd = np.sqrt(np.diag(got["cov_total"]))
    np.testing.assert_allclose(r32.sd.cpu().numpy(), sd, rtol=1e-15)
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_allclose(r32.corr.cpu().numpy(), got["cov_total"] / (sd[:, None] * sd[None, :]), rtol=1e-14)


@pytest.mark.parametrize("name", ["S5-C3-D64-f32", "S600-C2-D3-f64", "S4-C1025-D2-f32", "S9-C3-D17-f64", "offset-f64"])
def test_equal_bits_on_a_strided_view(name):
    """the same update sequence on a contiguous tensor and on a strided view of the same numbers: bit-identical state and results."""
    case = cases.BY_NAME[name]
    x = torch.from_numpy(cases.samples(case).copy()).to(DEV)
    big = torch.zeros((case.S, case.C + 5, case.D + 3), dtype=x.dtype, device=DEV)
    big[:, 2:case.C + 2, :case.D] = x
    view = big[:, 2:case.C + 2, :case.D]
    assert view.stride() != x.stride()
    for chunks in cases.chunkings(case.S):
        a, b = fed(x, chunks), fed(view, chunks)
        assert torch.equal(a.state.view(torch.int64), b.state.view(torch.int64))
        ra, rb = a.result(reg_n=5), b.result(reg_n=5)
        for f in ("mean", "sd", "cov_within", "cov_total", "corr", "rhat"):
            assert torch.equal(getattr(ra, f).view(torch.int64), getattr(rb, f).view(torch.int64)), f
        assert torch.equal(ra.inv_mass.view(torch.int32), rb.inv_mass.view(torch.int32))


@pytest.mark.parametrize("case", cases.CASES, ids=cases.IDS)
def test_the_bits_shared_with_running_moments(case):
    """the same feed into RunningMoments: its means, M2, mean, variances, R-hat and inv_mass are the means, the diagonal
    co-moments and the diagonals of RunningCovariance bit for bit (NaN where it has NaN)."""
    x = torch.from_numpy(cases.samples(case).copy()).to(DEV)
    iu, ju = cases.pairs(case.D)
    dg = torch.from_numpy(iu == ju).to(DEV)
    same = lambda a, b: np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)        # noqa: E731
    for chunks in cases.chunkings(case.S):
        a, b = fed(x, chunks), fed(x, chunks, cls=DG.RunningMoments)
        assert same(a.means, b.state[0]) and same(a.comoments[:, dg], b.state[1])
        for dtype in (torch.float32, torch.float64):
            ra, rb = a.result(reg_n=5, dtype=dtype), b.result(reg_n=5, dtype=dtype)
            assert same(ra.mean, rb.mean) and same(ra.rhat, rb.rhat) and same(ra.sd, rb.sd)
            assert same(ra.cov_within.diagonal(), rb.var_within) and same(ra.cov_total.diagonal(), rb.var_total)
            assert ra.inv_mass.dtype == dtype and same(ra.inv_mass.diagonal(), rb.inv_mass)


@pytest.mark.parametrize("name", ["S5-C3-D64-f32", "S600-C2-D3-f64", "S7-C65-D3-f64"])
def test_merge_equals_one_accumulator_fed_both(name):
    case = cases.BY_NAME[name]
    xn = cases.samples(case)
    x = torch.from_numpy(xn.copy()).to(DEV)
    k = max(1, case.S // 3)
    merged = DG.RunningCovariance().update(x[:k]).merge(DG.RunningCovariance().update(x[k:]))
    assert merged.n_draws == case.S
    inside(quantities(merged)[0], cases.restate(xn, (k, case.S - k)), case, xn, "merge")
    empty = DG.RunningCovariance().merge(merged)                       # into an accumulator without a shape: a copy
    assert empty.n_draws == case.S and torch.equal(empty.state, merged.state) and empty.state is not merged.state
    with pytest.raises(ValueError, match="merge"):
        merged.merge(DG.RunningCovariance(case.C + 1, case.D, DEV).update(torch.zeros(2, case.C + 1, case.D, device=DEV)))
    assert merged.reset().n_draws == 0 and merged.update(x).n_draws == case.S
    inside(quantities(merged)[0], cases.restate(xn, (case.S,)), case, xn, "after reset")


def test_stack_of_the_halves():
    """stack() of the accumulators of a run's halves: the restatement's stack (inside the band), with RunningMoments' split R-hat."""
    case = cases.BY_NAME["S600-C2-D3-f32"]
    xn = cases.samples(case)
    x = torch.from_numpy(xn.copy()).to(DEV)
    h = case.S // 2
    halves = DG.RunningCovariance.stack([DG.RunningCovariance().update(x[:h]), DG.RunningCovariance().update(x[h:])])
    assert halves.n_chains == 2 * case.C and halves.n_draws == h and halves.n_coordinates == case.D
    ref = cases.State.stack([cases.State().update(xn[:h]), cases.State().update(xn[h:])]).finish()
    inside(quantities(halves)[0], ref, case, xn, "stack")
    mom = DG.RunningMoments.stack([DG.RunningMoments().update(x[:h]), DG.RunningMoments().update(x[h:])]).result()
    assert torch.equal(halves.result().rhat, mom.rhat)
    with pytest.raises(ValueError, match="differ"):
        DG.RunningCovariance.stack([DG.RunningCovariance().update(x[:h]), DG.RunningCovariance().update(x[h + 1:])])


def test_one_nan_draw_poisons_its_own_pairs_only():
    """the NaN draw: NaN in the mean of its (chain, coordinate), in every co-moment of that chain that involves the coordinate
    and in that row and column of the pooled matrices, nowhere else - and it stays after later finite chunks."""
    case = cases.BY_NAME["nan-f64"]
    xn = cases.samples(case)
    x = torch.from_numpy(xn.copy()).to(DEV)
    _, c, d = cases.NAN_AT
    iu, ju = cases.pairs(case.D)
    bad_m = np.zeros((case.C, case.D), bool)
    bad_m[c, d] = True
    bad_q = np.zeros((case.C, iu.size), bool)
    bad_q[c] = (iu == d) | (ju == d)
    line = np.arange(case.D) == d
    for chunks in cases.chunkings(case.S):
        acc = fed(x, chunks)
        acc.update(torch.ones(3, case.C, case.D, dtype=x.dtype, device=DEV))
        got, _ = quantities(acc)
        assert np.array_equal(np.isnan(got["chain_mean"]), bad_m) and np.array_equal(np.isnan(got["chain_q"]), bad_q)
        for k in ("mean", "rhat"):
            assert np.array_equal(np.isnan(got[k]), line), k
        for k in MATRICES:
            assert np.array_equal(np.isnan(got[k]), line[:, None] | line[None, :]), k
    inf = x.clone()
    inf[cases.NAN_AT] = float("inf")
    got, _ = quantities(fed(inf, (case.S,)))
    assert np.array_equal(np.isnan(got["chain_mean"]), bad_m) and np.array_equal(np.isnan(got["chain_q"]), bad_q)
    merged = fed(x[:10], (10,)).merge(fed(x[10:], (10,)))                       # the torch merge keeps the rule
    got, _ = quantities(merged)
    assert np.array_equal(np.isnan(got["chain_mean"]), bad_m) and np.array_equal(np.isnan(got["chain_q"]), bad_q)


def test_cpu_in_cpu_out_and_one_chain():
    """host samples are staged and the results come back on the host; an [S, D] tensor is one chain."""
    case = cases.BY_NAME["S9-C3-D17-f32"]
    xn = cases.samples(case)
    acc = DG.RunningCovariance().update(torch.from_numpy(xn.copy()))
    assert acc.state.is_cuda
    r = acc.result(reg_n=5)
    assert r.mean.device.type == "cpu" and r.inv_mass.device.type == "cpu" and r.inv_mass.shape == (case.D, case.D) and r.corr.device.type == "cpu"
    ref = cases.restate(xn, (case.S,))
    np.testing.assert_allclose(r.cov_total.numpy(), ref["cov_total"], rtol=1e-12, atol=1e-12)
    assert r.to(DEV).cov_total.is_cuda and r.max_rhat() == pytest.approx(np.nanmax(ref["rhat"]), rel=1e-12)
    one = DG.RunningCovariance().update(torch.from_numpy(xn[:, 0].copy()).to(DEV)).result()
    assert one.n_chains == 1 and one.cov_total.is_cuda
    np.testing.assert_allclose(one.cov_total.cpu().numpy(), np.cov(xn[:, 0].astype(np.float64), rowvar=False), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(one.cov_within.cpu().numpy(), one.cov_total.cpu().numpy(), rtol=1e-14)
    half = DG.RunningCovariance().update(torch.from_numpy(xn.copy()).to(DEV).half()).result()           # half samples: exact in float32
    assert torch.isfinite(half.cov_total).all()
