"""GPU: diagnostics.RunningMoments (csrc/moments.hip) against the numpy restatement of tests/moments_cases.py on every case and
chunking, inside the band measured in tests/test_moments_cases_cpu.py (4 x what the restatement loses against longdouble, at
least 1e-15); merge, stack against diagnostics.summary, equal bits on strided views, and the NaN rule."""
import numpy as np
import pytest
import torch

import moments_cases as cases
from hamiltorch_amd import _abi
from hamiltorch_amd import diagnostics as DG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {np.float32: torch.float32, np.float64: torch.float64}


def quantities(acc):
    """A RunningMoments' state and result as the restatement's dict of numpy arrays."""
    r = acc.result(reg_n=cases.REG_N, reg_floor=cases.REG_FLOOR, dtype=torch.float64)
    out = dict(chain_mean=acc.state[0], chain_m2=acc.state[1], mean=r.mean, var_within=r.var_within, var_between=r.var_between,
               var_total=r.var_total, rhat=r.rhat, inv_mass=r.inv_mass)
    return {k: v.cpu().numpy() for k, v in out.items()}, r


def fed(x, chunks, form="tensor"):
    """The accumulator of x[S, C, D] (a device tensor) fed `chunks` rows at a time."""
    acc, r0 = DG.RunningMoments(), 0
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
        assert _abi.last_route() == "moments_update_kernel<%s>" % ("float" if case.dtype == np.float32 else "double")
        got, r = quantities(acc)
        assert (acc.n_draws, acc.n_chains, acc.n_coordinates) == (case.S, case.C, case.D) == (r.n_draws, r.n_chains, r.mean.numel())
        assert r.mean.device.type == "cuda" and r.inv_mass.dtype == torch.float64
        inside(got, ref, case, xn, "%s %s" % (case.name, chunks))
        inside(quantities(fed(x, chunks, "list"))[0], ref, case, xn, "%s %s list" % (case.name, chunks))
    # the strided view: one update(skip=2) of the chain slice, = the restatement fed all rows at once
    view = big[:, 1:case.C + 1, :case.D]
    assert not view.is_contiguous()
    acc = DG.RunningMoments(case.C, case.D, DEV).update(view, skip=2)
    inside(quantities(acc)[0], cases.restate(xn, (case.S,)), case, xn, "%s view" % case.name)
    r32 = acc.result(reg_n=cases.REG_N)
    assert r32.inv_mass.dtype == torch.float32 and acc.result().inv_mass is None
    got = quantities(acc)[0]
    np.testing.assert_array_equal(r32.inv_mass.cpu().numpy(), got["inv_mass"].astype(np.float32))        # the float32 output: the fp64 value, rounded once
    np.testing.assert_allclose(r32.sd.cpu().numpy(), np.sqrt(got["var_total"]), rtol=1e-15)


@pytest.mark.parametrize("name", ["S33-C64-D130-f32", "S600-C2-D3-f64", "S4-C1025-D2-f32", "offset-f64"])
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
        for f in ("mean", "sd", "var_within", "var_between", "var_total", "rhat"):
            assert torch.equal(getattr(ra, f).view(torch.int64), getattr(rb, f).view(torch.int64)), f
        assert torch.equal(ra.inv_mass.view(torch.int32), rb.inv_mass.view(torch.int32))


@pytest.mark.parametrize("name", ["S33-C64-D130-f32", "S600-C2-D3-f64", "S7-C65-D3-f64"])
def test_merge_equals_one_accumulator_fed_both(name):
    case = cases.BY_NAME[name]
    xn = cases.samples(case)
    x = torch.from_numpy(xn.copy()).to(DEV)
    k = case.S // 3
    merged = DG.RunningMoments().update(x[:k]).merge(DG.RunningMoments().update(x[k:]))
    assert merged.n_draws == case.S
    inside(quantities(merged)[0], cases.restate(xn, (k, case.S - k)), case, xn, "merge")
    empty = DG.RunningMoments().merge(merged)                          # into an accumulator without a shape: a copy
    assert empty.n_draws == case.S and torch.equal(empty.state, merged.state) and empty.state is not merged.state
    with pytest.raises(ValueError, match="merge"):
        merged.merge(DG.RunningMoments(case.C + 1, case.D, DEV).update(torch.zeros(2, case.C + 1, case.D, device=DEV)))
    assert merged.reset().n_draws == 0 and merged.update(x).n_draws == case.S
    inside(quantities(merged)[0], cases.restate(xn, (case.S,)), case, xn, "after reset")


def test_stack_of_the_halves_is_split_rhat():
    """an even-S run: stack() of the accumulators of its halves has summary()'s split R-hat (inside the band of the case); the
    whole run's mean is summary()'s.  summary()'s sd is sqrt(var_plus) = sqrt((n - 1) / n W + B), not the pooled sqrt(var_total)
    that RunningMoments reports as sd: what is compared with it is that expression of var_within and var_between."""
    case = cases.BY_NAME["S600-C2-D3-f32"]
    xn = cases.samples(case)
    x = torch.from_numpy(xn.copy()).to(DEV)
    s = DG.summary(x)
    h = case.S // 2
    halves = DG.RunningMoments.stack([DG.RunningMoments().update(x[:h]), DG.RunningMoments().update(x[h:])])
    assert halves.n_chains == 2 * case.C and halves.n_draws == h
    band = cases.band(case)
    rh = halves.result().rhat
    assert float(((rh - s.rhat).abs() / s.rhat).max()) <= band["rhat"]
    r = DG.RunningMoments().update(x).result()
    scale = float(np.abs(xn).max())
    assert float((r.mean - s.mean).abs().max()) / scale <= band["mean"]
    n = float(case.S)
    var_plus = (n - 1.0) / n * r.var_within + r.var_between
    assert float(((var_plus.sqrt() - s.sd).abs() / s.sd).max()) <= band["var_within"] + band["var_between"]
    assert float(((r.sd - r.var_total.sqrt()).abs()).max()) == 0.0
    with pytest.raises(ValueError, match="differ"):
        DG.RunningMoments.stack([DG.RunningMoments().update(x[:h]), DG.RunningMoments().update(x[h + 1:])])


def test_one_nan_draw_poisons_its_own_chain_only():
    """the NaN draw: NaN in the mean and M2 of its (chain, coordinate) and in that coordinate's pooled outputs, nowhere else - and
    it stays after later finite chunks."""
    case = cases.BY_NAME["nan-f64"]
    xn = cases.samples(case)
    x = torch.from_numpy(xn.copy()).to(DEV)
    _, c, d = cases.NAN_AT
    bad = np.zeros((case.C, case.D), bool)
    bad[c, d] = True
    for chunks in cases.chunkings(case.S):
        acc = fed(x, chunks)
        acc.update(torch.ones(3, case.C, case.D, dtype=x.dtype, device=DEV))
        got, _ = quantities(acc)
        assert np.array_equal(np.isnan(got["chain_mean"]), bad) and np.array_equal(np.isnan(got["chain_m2"]), bad)
        for k in ("mean", "var_within", "var_between", "var_total", "rhat", "inv_mass"):
            assert np.array_equal(np.isnan(got[k]), np.arange(case.D) == d), k
    inf = x.clone()
    inf[cases.NAN_AT] = float("inf")
    got, _ = quantities(fed(inf, (case.S,)))
    assert np.array_equal(np.isnan(got["chain_mean"]), bad) and np.array_equal(np.isnan(got["chain_m2"]), bad)


def test_cpu_in_cpu_out_and_one_chain():
    """host samples are staged and the results come back on the host; an [S, D] tensor is one chain."""
    case = cases.BY_NAME["S33-C64-D130-f32"]
    xn = cases.samples(case)
    acc = DG.RunningMoments().update(torch.from_numpy(xn.copy()))
    assert acc.state.is_cuda
    r = acc.result(reg_n=5)
    assert r.mean.device.type == "cpu" and r.inv_mass.device.type == "cpu" and r.inv_mass.shape == (case.D,)
    ref = cases.restate(xn, (case.S,))
    np.testing.assert_allclose(r.var_total.numpy(), ref["var_total"], rtol=1e-12)
    one = DG.RunningMoments().update(torch.from_numpy(xn[:, 0].copy()).to(DEV)).result()
    assert one.n_chains == 1 and float(one.var_between.abs().max()) == 0.0
    np.testing.assert_allclose(one.var_total.cpu().numpy(), xn[:, 0].astype(np.float64).var(axis=0, ddof=1), rtol=1e-12)
    half = DG.RunningMoments().update(torch.from_numpy(xn.copy()).to(DEV).half()).result()           # half samples: exact in float32
    assert torch.isfinite(half.mean).all()
