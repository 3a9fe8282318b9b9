"""GPU: the compiled callback code op by op (cases in tests/jit_op_cases.py) against torch.autograd.

* every Hessian-capable case through rmhmc._CompiledCurvature (csrc/jit/derivs_callback.hip.in): value, gradient, -Hessian and the
  third-derivative contraction with all rows as chains of one launch - float64 against autograd in float64 (the CPU rule, or the
  case's stated bound where ocml's special functions differ from glibc by a few ulp), float32 against autograd of the callable in
  float32 (the case's bound, default 1e-5 (1 + |ref|)); non-finite entries exactly;
* the cases whose Hessian the graph cannot form (lgamma / digamma): sample() on the compiled HMC kernel against the torch-evaluated
  callback path (HAMILTORCH_AMD_JIT=0), float64, the same seeds, chains started on the edge rows;
* end to end: -||w|| - w.w / 2 and a relu target from params_init = 0 stay compiled and equal the callback path.
"""
import numpy as np
import pytest
import torch

from jit_op_cases import CASES, CASE_BY_NAME
from test_jit_ops import assert_parity, autograd_derivs

pytestmark = pytest.mark.gpu
HESS = [c for c in CASES if c.refuse is None and c.hess]
NO_HESS = ["lgamma", "digamma_value", "distributions_lgamma"]


@pytest.fixture(scope="module")
def ht():
    import hamiltorch_amd
    assert torch.cuda.is_available()
    return hamiltorch_amd


def route():
    from hamiltorch_amd import _abi
    return _abi.last_route()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("c", HESS, ids=[c.name for c in HESS])
def test_compiled_derivatives_equal_autograd(ht, c, dtype):
    from hamiltorch_amd import jit, rmhmc
    rows = c.rows if dtype == torch.float64 else c.f32_rows
    assert rows, c.name
    dev = torch.device("cuda:0")
    theta = torch.tensor(rows, dtype=dtype, device=dev)
    example = torch.tensor(c.example_point, dtype=dtype)          # (on the CPU: the cases build their constants there)
    cv = rmhmc._CompiledCurvature(c.fn, jit.compile_derivs(c.fn, example, dtype, fresh=True), theta)
    g, nH = cv.grad_neg_hessian(theta)
    lp = cv.value(theta)
    assert "hta_cb_derivs_kernel<D=%d" % c.D in route(), route()
    D = c.D
    M = np.random.default_rng(7).standard_normal((len(rows), D, D))
    M = 0.5 * (M + np.swapaxes(M, 1, 2))
    con = cv.contract(theta, torch.tensor(M, dtype=dtype, device=dev)).cpu().double().numpy() if c.third else None
    lp, g, H = lp.cpu().double().numpy(), g.cpu().double().numpy(), -nH.cpu().double().numpy()
    if dtype == torch.float64:
        tol = max(c.tol_cpu, c.rtol64 or 0.0)
        order = 3 if c.third else 2
    else:
        tol, order = c.tol32, 2
    for k, row in enumerate(rows):
        o = 1 if row in c.grad_only_rows else order
        ref = autograd_derivs(c.fn, row, o, dtype)
        if not (np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()):
            o = 1
        what = "%s %s at %s" % (c.name, str(dtype)[6:], row)
        assert_parity(lp[k:k + 1], ref[0], tol, what + ", value")
        assert_parity(g[k], ref[1], tol, what + ", gradient")
        if o >= 2:
            assert_parity(H[k], ref[2], tol, what + ", Hessian")
        if o >= 3:
            want = np.einsum("ijk,ij->k", ref[3], M[k])
            assert_parity(con[k], want, 10 * tol, what + ", contraction")


def _both_routes(ht, monkeypatch, fn, th0, **kw):
    a = torch.stack(list(ht.sample(fn, th0, **kw)))
    r = route()
    monkeypatch.setenv("HAMILTORCH_AMD_JIT", "0")
    b = torch.stack(list(ht.sample(fn, th0, **kw)))
    assert "hta_cb_hmc_kernel" not in route()
    monkeypatch.delenv("HAMILTORCH_AMD_JIT")
    return a, b, r


@pytest.mark.parametrize("name", NO_HESS)
def test_no_hessian_cases_sample_like_the_callback_path(ht, monkeypatch, name):
    """lgamma / digamma: the compiled HMC trajectory kernel against the callback path, float64, chain by chain, from the edge rows."""
    c = CASE_BY_NAME[name]
    starts = [c.example_point] + [r for r in c.rows if all(np.isfinite(c.fn(torch.tensor(r, dtype=torch.float64)).detach().numpy().reshape(-1)))]
    th0 = torch.tensor(starts, dtype=torch.float64, device="cuda:0").repeat(4, 1)
    kw = dict(num_samples=6, num_steps_per_sample=4, step_size=0.01, verbose=False, seed=5)
    a, b, r = _both_routes(ht, monkeypatch, _on_device(c.fn), th0, **kw)
    assert "hta_cb_hmc_kernel<D=%d" % c.D in r, r
    err = (a - b).abs().amax(dim=(0, 2))
    assert float(err.max()) <= 1e-9, float(err.max())


def test_norm_target_leaves_zero(ht, monkeypatch):
    """-||w|| - w.w / 2 from params_init = 0: the gradient at the zero norm is 0 (torch's), not NaN - compiled, the chains leave 0 and
    equal the callback path chain by chain."""
    fn = lambda w: -torch.linalg.vector_norm(w) - 0.5 * (w * w).sum()  # noqa: E731
    th0 = torch.zeros(64, 3, dtype=torch.float64, device="cuda:0")
    a, b, r = _both_routes(ht, monkeypatch, fn, th0, num_samples=8, num_steps_per_sample=5, step_size=0.2, verbose=False, seed=11)
    assert "hta_cb_hmc_kernel<D=3" in r, r
    assert torch.isfinite(a).all() and float(a[-1].abs().amax(dim=1).min()) > 0
    assert float((a - b).abs().max()) <= 1e-9


def test_relu_target_from_zero_stays_compiled(ht, monkeypatch):
    """A relu target from params_init = 0: the example check at 0 now agrees with autograd (derivative 0 at the kink), so the run stays on
    the compiled kernel, and equals the callback path."""
    fn = lambda w: -0.5 * (w * w).sum() - torch.relu(w).sum()  # noqa: E731
    th0 = torch.zeros(64, 2, dtype=torch.float64, device="cuda:0")
    a, b, r = _both_routes(ht, monkeypatch, fn, th0, num_samples=8, num_steps_per_sample=5, step_size=0.2, verbose=False, seed=12)
    assert "hta_cb_hmc_kernel<D=2" in r, r
    assert float((a - b).abs().max()) <= 1e-9


def _on_device(fn):
    """The case callables build their constants on the CPU; sample() calls them with device tensors."""
    def f(w):
        with torch.device(w.device):
            return fn(w)
    return f
