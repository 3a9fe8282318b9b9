"""CPU: the callback compiler op by op against torch.autograd (cases in tests/jit_op_cases.py) - no GPU needed.

* coverage: every key of trace.lowering_table() is reached by some case's trace, or listed in EXCLUDED with the reason;
  no excluded key is reached;
* parity: value, gradient, Hessian (and the third derivatives of the smooth cases) of the lowered graph (ir.Graph.evaluate,
  float64 - what the device computes up to rounding) against torch.autograd of the callable in float64, row by row, at kinks,
  ties, tails, zeros and poles: finite entries to 1e-12 (1 + |ref|), non-finite entries exactly (NaN for NaN, inf of the same sign);
  higher derivatives where torch's value and gradient are finite and the case does not list the row in `grad_only_rows`;
  what must be refused raises ir.Unsupported with its reason; on the rows with inf / NaN inputs the model in float32 too;
* hipRTC: every case builds for gfx950 in both dtypes (the derivative skeleton where the Hessian exists, the HMC skeleton
  otherwise), nothing spilled.
"""
import numpy as np
import pytest
import torch

from hamiltorch_amd.jit import runtime, trace
from hamiltorch_amd.jit.ir import Unsupported
from hamiltorch_amd.jit.trace import trace_callback

from jit_op_cases import CASES
from test_jit_cpu import _symbols

f64 = torch.float64
LIVE = [c for c in CASES if c.refuse is None]
REFUSED = [c for c in CASES if c.refuse is not None]

# table keys no case reaches, each with the reason
_OUT = "`.out` overload: make_fx never emits it"
_COMPOSITE = "CompositeImplicitAutograd: make_fx records the ops it decomposes into"
_COPY = "`_copy` variant: functionalize(remove='mutations') keeps the view op"
EXCLUDED = {
    **{k: _OUT for k in ("aten.clone.out", "aten.lift_fresh_copy.out", "aten.alias_copy.out", "aten.detach_copy.out", "aten._to_copy.out",
                         "aten.scalar_tensor.out", "aten.zeros_like.out", "aten.empty_like.out", "aten.ones_like.out", "aten.full_like.out",
                         "aten.new_zeros.out", "aten.new_empty.out", "aten.new_ones.out", "aten.new_full.out", "aten._unsafe_view.out",
                         "aten.permute_copy.out", "aten.t_copy.out", "aten.unsqueeze_copy.out", "aten.expand_copy.out", "aten.diag_embed.out",
                         "aten.flip.out", "aten.repeat.out")},
    **{k: _COPY for k in ("aten.alias_copy.default", "aten.detach_copy.default", "aten.view_copy.default", "aten.permute_copy.default",
                          "aten.transpose_copy.int", "aten.t_copy.default", "aten.unsqueeze_copy.default", "aten.squeeze_copy.default",
                          "aten.squeeze_copy.dim", "aten.squeeze_copy.dims", "aten.expand_copy.default", "aten.select_copy.int",
                          "aten.slice_copy.Tensor", "aten.unbind_copy.int", "aten.split_copy.Tensor",
                          "aten.split_with_sizes_copy.default")},
    **{k: _COMPOSITE for k in (
        "aten.__and__.Tensor", "aten.__or__.Tensor", "aten.absolute.default", "aten.adjoint.default", "aten.arctan.default",
        "aten.broadcast_to.default", "aten.chunk.default", "aten.clip.default", "aten.concat.default", "aten.conj.default",
        "aten.contiguous.default", "aten.diag.default", "aten.expand_as.default", "aten.flatten.using_ints", "aten.ger.default",
        "aten.greater.Scalar", "aten.greater.Tensor", "aten.greater_equal.Scalar", "aten.greater_equal.Tensor", "aten.inner.default",
        "aten.isfinite.default", "aten.less.Scalar", "aten.less.Tensor", "aten.less_equal.Scalar", "aten.less_equal.Tensor",
        "aten.linear.default", "aten.log_sigmoid.default", "aten.log_softmax.int", "aten.mH.default", "aten.mT.default",
        "aten.matmul.default", "aten.max.other", "aten.min.other", "aten.narrow.default", "aten.negative.default",
        "aten.not_equal.Scalar", "aten.not_equal.Tensor", "aten.outer.default", "aten.positive.default", "aten.reshape.default",
        "aten.resolve_conj.default", "aten.resolve_neg.default", "aten.softmax.int", "aten.special_erf.default",
        "aten.special_erfc.default", "aten.square.default", "aten.std.default", "aten.std.dim", "aten.to.device", "aten.to.dtype",
        "aten.to.dtype_layout", "aten.to.other", "aten.true_divide.Scalar", "aten.true_divide.Tensor", "aten.type_as.default",
        "aten.var.default", "aten.var.dim", "aten.where.Scalar", "aten.where.ScalarOther", "aten.where.ScalarSelf")},
    "aten.mH.a": "Dimname-style alias overload of mH: no schema of its own to dispatch, never emitted",
    "aten.mT.a": "Dimname-style alias overload of mT: no schema of its own to dispatch, never emitted",
    "aten.view_as_real.default": "complex input only: a real callable never produces one",
    "aten._conj.default": "complex input only: conj of a real tensor is not dispatched",
    "aten.detach_.default": "in-place: functionalize records aten.detach instead",
    "aten._assert_tensor_metadata.default": "emitted by `.to()` under pre-dispatch export only, not by make_fx",
    "aten.lift_fresh.default": "its operand is a constant: torch folds it (trace._fold_constant) before the table is consulted",
    "aten.lift_fresh_copy.default": "its operand is a constant: torch folds it (trace._fold_constant) before the table is consulted",
}


def _table_names():
    return {str(k): k for k in trace.lowering_table()}


# ---- torch.autograd, float64 --------------------------------------------------------------------------------------------
def autograd_derivs(fn, row, order, dtype=f64):
    """value, gradient, Hessian (order >= 2), third derivatives (order 3) of fn at one row (float64 arrays of autograd in `dtype`);
    zeros where autograd has no path."""
    x = torch.tensor(row, dtype=dtype, requires_grad=True)
    D = x.numel()
    v = fn(x)
    v = v.sum() if v.dim() else v
    g, = torch.autograd.grad(v, x, create_graph=order > 1, allow_unused=True)
    g = torch.zeros_like(x) if g is None else g
    out = [np.array([float(v)]), g.detach().double().numpy()]
    if order > 1:
        H = []
        for i in range(D):
            if g[i].requires_grad:
                h, = torch.autograd.grad(g[i], x, create_graph=order > 2, retain_graph=True, allow_unused=True)
            else:
                h = None
            H.append(torch.zeros_like(x) if h is None else h)
        out.append(torch.stack(H).detach().double().numpy())
        if order > 2:
            T3 = np.zeros((D, D, D))
            for i in range(D):
                for j in range(D):
                    if H[i][j].requires_grad:
                        t, = torch.autograd.grad(H[i][j], x, retain_graph=True, allow_unused=True)
                        T3[i, j] = 0 if t is None else t.double().numpy()
            out.append(T3)
    return out


def graph_derivs(tr, rows, order):
    g = tr.graph
    D = tr.D
    grads = tr.grad()
    outs = [tr.value] + grads
    if order > 1:
        H = [g.grad(gi) for gi in grads]
        outs += [H[i][j] for i in range(D) for j in range(D)]
        if order > 2:
            outs += [t for i in range(D) for j in range(D) for t in g.grad(H[i][j])]
    ev = g.evaluate(outs, np.asarray(rows, np.float64), np.float64)
    res = []
    for r in ev:
        parts = [r[:1], r[1:1 + D]]
        if order > 1:
            parts.append(r[1 + D:1 + D + D * D].reshape(D, D))
            if order > 2:
                parts.append(r[1 + D + D * D:].reshape(D, D, D))
        res.append(parts)
    return res


def assert_parity(got, ref, tol, what):
    """Finite reference entries to tol * (1 + |ref|); non-finite ones exactly (NaN for NaN, +-inf with the sign)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    bad = np.zeros(ref.shape, bool)
    with np.errstate(invalid="ignore"):
        bad[fin] = ~(np.abs(got[fin] - ref[fin]) <= tol * (1.0 + np.abs(ref[fin])))
    nan = np.isnan(ref)
    bad[nan] = ~np.isnan(got[nan])
    inf = np.isinf(ref)
    bad[inf] = got[inf] != ref[inf]
    assert not bad.any(), "%s: got %s, torch %s" % (what, got[bad], ref[bad])


def order_of(c):
    return 3 if c.third else (2 if c.hess else 1)


# ---- tests ----------------------------------------------------------------------------------------------------------------
def test_every_table_key_is_reached_or_excluded(monkeypatch):
    table = dict(trace.lowering_table())
    reached = set()

    def recording(key, fn):
        def wrapper(*a, **k):
            reached.add(str(key))
            return fn(*a, **k)
        return wrapper
    monkeypatch.setattr(trace, "_TABLE", {k: recording(k, fn) for k, fn in table.items()})
    for c in CASES:
        try:
            trace_callback(c.fn, torch.tensor(c.example_point, dtype=f64))
        except Unsupported:
            assert c.refuse is not None, c.name
    names = set(_table_names())
    assert len(names) == len(table)
    missing = sorted(names - reached - set(EXCLUDED))
    assert not missing, "table keys no case reaches and EXCLUDED does not list: %s" % missing
    wrongly = sorted(reached & set(EXCLUDED))
    assert not wrongly, "excluded keys a case reaches: %s" % wrongly
    assert set(EXCLUDED) <= names, sorted(set(EXCLUDED) - names)


@pytest.mark.parametrize("c", LIVE, ids=[c.name for c in LIVE])
def test_graph_equals_autograd(c):
    tr = trace_callback(c.fn, torch.tensor(c.example_point, dtype=f64))
    order = order_of(c)
    got = graph_derivs(tr, c.rows, order)
    for row, mine in zip(c.rows, got):
        o = 1 if row in c.grad_only_rows else order
        ref = autograd_derivs(c.fn, row, o)
        if not (np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()):
            o = 1           # (a non-finite value or gradient: torch's double backward multiplies it by zeros - NaN everywhere)
        for k, what in enumerate(("value", "gradient", "Hessian", "third derivatives")[:o + 1]):
            assert_parity(mine[k], ref[k], c.tol_cpu, "%s at %s, %s" % (c.name, row, what))


NONFINITE32 = [c for c in LIVE if "nan_to_num" in c.name or any(not np.isfinite(v) for r in c.f32_rows for v in r)]


@pytest.mark.parametrize("c", NONFINITE32, ids=[c.name for c in NONFINITE32])
def test_graph_in_float32_equals_autograd_in_float32(c):
    """The numpy model in float32 on inf / NaN inputs (and nan_to_num's float32 largest finite value, ir.Graph.finfo_max) against
    autograd of the callable in float32: value and gradient, the case's float32 bound, non-finite entries exactly."""
    tr = trace_callback(c.fn, torch.tensor(c.example_point, dtype=torch.float32))
    out = tr.graph.evaluate([tr.value] + tr.grad(), np.asarray(c.f32_rows, np.float32))
    assert out.dtype == np.float32
    for row, mine in zip(c.f32_rows, out.astype(np.float64)):
        ref = autograd_derivs(c.fn, row, 1, torch.float32)
        assert_parity(mine[:1], ref[0], c.tol32, "%s float32 at %s, value" % (c.name, row))
        assert_parity(mine[1:], ref[1], c.tol32, "%s float32 at %s, gradient" % (c.name, row))


@pytest.mark.parametrize("c", REFUSED, ids=[c.name for c in REFUSED])
def test_refused_with_a_reason(c):
    with pytest.raises(Unsupported) as e:
        tr = trace_callback(c.fn, torch.tensor(c.example_point, dtype=f64))
        tr.grad()
    assert c.refuse in str(e.value) and str(e.value), str(e.value)


def test_lgamma_hessian_is_refused():
    """The lgamma family cannot form a Hessian (digamma' is not lowered): refused with the reason, not another exception."""
    from jit_op_cases import CASE_BY_NAME
    c = CASE_BY_NAME["lgamma"]
    tr = trace_callback(c.fn, torch.tensor(c.example_point, dtype=f64))
    with pytest.raises(Unsupported, match="digamma"):
        runtime.derivs_generated_source(tr, f64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_every_case_builds_for_gfx950(dtype, tmp_path):
    """hipRTC builds each case: the derivative kernels where the Hessian exists, the HMC trajectory kernel otherwise; no spills."""
    for c in LIVE:
        tr = trace_callback(c.fn, torch.tensor(c.example_point, dtype=f64))
        if c.hess:
            src, skel, kern = runtime.derivs_generated_source(tr, dtype), runtime.SKELETON_DERIVS, "hta_cb_derivs_kernel"
        else:
            src, skel, kern = runtime.hmc_generated_source(tr, dtype, 0), runtime.SKELETON_HMC, "hta_cb_hmc_kernel"
        key, blob = runtime.compile_source(src, skel)
        sym, regs = _symbols(blob, tmp_path)
        assert kern in sym, (c.name, kern)
        assert regs["vgpr_spill_count"] == 0 and regs["private_segment_fixed_size"] == 0, (c.name, regs)
