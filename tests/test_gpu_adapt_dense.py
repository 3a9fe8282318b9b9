"""GPU: hamiltorch_amd.warmup(mass="dense") on the engines - the rotated Gaussian on the Gaussian kernels and the rotated product
of hyperbolic secants as a compiled closure, held to the conditions tests/test_adapt_dense_cpu.py holds the CPU oracle's own run
to (tests/dense_adapt_cases.py: check), with the GPU's own diagonal warm-up as the ESS baseline; shapes, dtypes and devices of
the result; the device-side refusal of a bad matrix; the D limit."""
import numpy as np
import pytest
import torch

import dense_adapt_cases as DA
import hamiltorch_amd as ht
from hamiltorch_amd import _abi, adapt
from hamiltorch_amd import diagnostics as DG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def follow_up(f, r, t, steps):
    out, acc = ht.sample(f, r.params, num_samples=DA.ROWS, num_steps_per_sample=steps, step_size=r.step_size, inv_mass=r.inv_mass, debug=2,
                         verbose=False, seed=t.seed + DA.FOLLOW_UP_SEED_INDEX)
    route = _abi.last_route()                                                   # (before summary() dispatches its own kernels)
    return DG.summary(out, skip=1), float(acc.mean()), route


def run(f, t, route):
    """The dense and the diagonal warm-up of `f` with the seeds of target `t`, their follow-ups, and the conditions."""
    D = t.scale.size
    start = torch.from_numpy(DA.start(t)).to(DEV)
    r = ht.warmup(f, start, num_steps_per_sample=DA.L, step_size=t.eps0, seed=t.seed, mass="dense")
    assert route in _abi.last_route(), _abi.last_route()
    assert r.params.shape == (DA.CHAINS, D) and r.params.is_cuda and r.params.dtype == torch.float32
    assert r.inv_mass.shape == (D, D) and r.inv_mass.dtype == torch.float32 and r.inv_mass.is_cuda and torch.equal(r.inv_mass, r.inv_mass.T)
    blocks = [h for h in r.history if h["kind"] == "block"]
    wins = [h for h in r.history if h["kind"] == "window"]
    assert len(blocks) == 45 and [h["n_draws"] for h in wins] == [45, 45, 90, 180]
    s, acc, route_dense = follow_up(f, r, t, DA.L_DENSE)
    diag = ht.warmup(f, start, num_steps_per_sample=DA.L, step_size=t.eps0, seed=t.seed)
    assert diag.inv_mass.shape == (D,)
    sd, _, _ = follow_up(f, diag, t, DA.L)
    print("step size dense %.4f diagonal %.4f | diagonal follow-up: rhat %.3f | %s" % (r.step_size, diag.step_size, sd.max_rhat(), route_dense))
    DA.check(t.name, [bool(h["accepted"]) for h in wins], DA.whitened_eigenvalues(t, r.inv_mass.double().cpu().numpy()), acc, s.max_rhat(), s.min_ess(),
             sd.min_ess())
    return route_dense


def test_dense_warmup_on_the_rotated_gaussian():
    """sd = (0.05, 0.2, 0.5, 1, 2, 5) along the columns of a rotation, float32, 64 chains from N(0, 1) starts, eps0 = 0.01."""
    t = DA.GAUSS
    tgt = ht.GaussianTarget(torch.zeros(6, device=DEV), precision=torch.from_numpy(DA.precision(t)).float().to(DEV))
    route = run(tgt, t, "hmc_gauss")
    assert "hmc_gauss" in route, route


def test_dense_warmup_on_a_compiled_closure():
    """log p = -sum_k log cosh((Q^T theta)_k / s_k), s = (0.05, 0.3, 1, 4), float32: an opaque callable, compiled into the
    trajectory kernel with a full mass (log cosh z written as |z| + log1p(exp(-2 |z|)): cosh overflows float32 at z = 89)."""
    t = DA.SECH
    s_ = torch.tensor(t.scale, dtype=torch.float32, device=DEV)
    Qt = torch.from_numpy(DA.rotation(t).T.copy()).float().to(DEV)

    def f(th):
        z = torch.abs(torch.mv(Qt, th) / s_)
        return -(z + torch.log1p(torch.exp(-2.0 * z))).sum()

    route = run(f, t, "hta_cb_hmc_kernel")
    assert "hta_cb_hmc_kernel" in route and "mass=2" in route, route


def test_one_chain_and_host_starts():
    """a (D,) start is one chain: (D,) params and a (D, D) mass back; a (C, D) start on the host: everything back on the host."""
    P = torch.tensor([[4.0, 1.0, 0.0], [1.0, 1.0, 0.2], [0.0, 0.2, 0.5]])
    tgt = ht.GaussianTarget(torch.zeros(3, device=DEV), precision=P.to(DEV))
    kw = dict(num_steps_per_sample=5, step_size=0.05, seed=3, block=5, windows=(2, 2), settle=1, mass="dense")
    one = ht.warmup(tgt, torch.zeros(3, device=DEV), **kw)
    assert one.params.shape == (3,) and one.params.is_cuda and one.inv_mass.shape == (3, 3) and one.inv_mass.is_cuda and one.step_size > 0
    assert len([h for h in one.history if h["kind"] == "block"]) == 5
    host = ht.warmup(ht.GaussianTarget(torch.zeros(3), precision=P), torch.zeros(16, 3), **kw)
    assert host.params.shape == (16, 3) and not host.params.is_cuda and not host.inv_mass.is_cuda and host.inv_mass.shape == (3, 3)
    assert all(not v.is_cuda for h in host.history for v in h.values() if torch.is_tensor(v))
    assert bool(torch.isfinite(host.inv_mass).all()) and bool((torch.linalg.eigvalsh(host.inv_mass.double()) > 0).all())
    tgt64 = ht.GaussianTarget(torch.zeros(3, device=DEV, dtype=torch.float64), precision=P.double().to(DEV))
    wide = ht.warmup(tgt64, torch.zeros(16, 3, device=DEV, dtype=torch.float64), **kw)
    assert wide.inv_mass.dtype == torch.float64 and wide.params.dtype == torch.float64
    plain = ht.warmup(tgt, torch.zeros(16, 3, device=DEV), adapt_mass=False, **kw)
    assert plain.inv_mass is None and not [h for h in plain.history if h["kind"] == "window"]


def test_a_refused_matrix_on_the_device_keeps_the_previous_one():
    """Controller.observe_window with device matrices: checked (finite, positive definite) and replaced without a read-back -
    `accepted` stays a 0-d bool tensor on the device."""
    ctl = adapt.Controller(0.1, block=1, windows=(1,) * 5, settle=0, mass="dense")
    mk = lambda a: torch.tensor(a, device=DEV)                                  # noqa: E731
    good = mk([[2.0, 0.5], [0.5, 1.0]])
    masses = [mk([[1.0, float("nan")], [float("nan"), 1.0]]), good, mk([[1.0, 2.0], [2.0, 1.0]]), mk([[float("inf"), 0.0], [0.0, 1.0]]),
              mk([[1.0, 0.0], [0.0, 0.0]])]
    seen = []
    for m in masses:
        ctl.next_block()
        ctl.observe_block(0.8)
        ctl.observe_window(m)
        seen.append(ctl.inv_mass.clone())
    wins = [h["accepted"] for h in ctl.history if h["kind"] == "window"]
    assert all(torch.is_tensor(a) and a.is_cuda and a.dim() == 0 and a.dtype == torch.bool for a in wins)
    assert torch.equal(seen[0], torch.eye(2, device=DEV)) and all(torch.equal(s, good) for s in seen[1:])
    assert [bool(a) for a in wins] == [False, True, False, False, False]


def test_d_over_the_limit_raises():
    f = lambda th: -(th * th).sum()                                             # noqa: E731
    with pytest.raises(ValueError, match="D <= 256"):
        ht.warmup(f, torch.zeros(4, DG.COVARIANCE_MAX_D + 1, device=DEV), mass="dense")
    with pytest.raises(ValueError, match="limit of 256"):
        DG.RunningCovariance().update(torch.zeros(3, 4, 257, device=DEV))
