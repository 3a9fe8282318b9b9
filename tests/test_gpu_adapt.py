"""GPU: hamiltorch_amd.warmup / adapt.warmup_with on the engines - the anisotropic Gaussian on the Gaussian kernels, a compiled
closure, host and one-chain starts, and a lambda around sample_model.  The conditions on the adapted mass, the acceptance, R-hat
and ESS are those tests/test_adapt_cpu.py holds the CPU oracle's own run to (there the ESS ratios to the HMC_NUTS baseline are
100 x and 16 x; a tenth and a quarter of them are the bars here)."""
import math

import numpy as np
import pytest
import torch

import adapt_cases as A
import hamiltorch_amd as ht
from hamiltorch_amd import _abi, adapt
from hamiltorch_amd import diagnostics as DG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def follow_up(f, r, seed, **kw):
    out, acc = ht.sample(f, r.params, num_samples=A.ROWS, num_steps_per_sample=A.L, step_size=r.step_size, inv_mass=r.inv_mass, debug=2,
                         verbose=False, seed=seed, **kw)
    return DG.summary(out, skip=1), float(acc.mean())


def nuts_baseline(f, t, start):
    """Sampler.HMC_NUTS with the same budget (burn = 450, 650 trajectories), identity mass, from the same start."""
    out = ht.sample(f, start, num_samples=A.BURN + A.ROWS, num_steps_per_sample=A.L, step_size=t.eps0, burn=A.BURN, sampler=ht.Sampler.HMC_NUTS,
                    verbose=False, seed=t.seed)
    return DG.summary(out, skip=1)


def test_warmup_on_the_anisotropic_gaussian():
    """sd = (0.05, 0.5, 1, 5), float32, 64 chains from N(0, 1) starts, eps0 = 0.01, the default schedule of 450 trajectories."""
    t = A.GAUSS
    sd = torch.tensor(t.scale, dtype=torch.float32, device=DEV)
    tgt = ht.GaussianTarget(torch.zeros(4, device=DEV), precision=torch.diag(1.0 / (sd * sd)))
    start = torch.from_numpy(A.start(t)).to(DEV)
    r = ht.warmup(tgt, start, num_steps_per_sample=A.L, step_size=t.eps0, seed=t.seed)
    assert "hmc_gauss" in _abi.last_route(), _abi.last_route()
    assert r.params.shape == (A.CHAINS, 4) and r.params.is_cuda and r.inv_mass.shape == (4,) and r.inv_mass.dtype == torch.float32 and r.inv_mass.is_cuda
    blocks = [h for h in r.history if h["kind"] == "block"]
    wins = [h for h in r.history if h["kind"] == "window"]
    assert len(blocks) == 45 and [h["n_draws"] for h in wins] == [45, 45, 90, 180] and all(bool(h["accepted"]) for h in wins)
    ratio = r.inv_mass.double().cpu().numpy() / t.variance
    ref, ctl = A.oracle_warmup(t, np.float32)                                   # the oracle-driven run of the same seeds
    ref_blocks = [h for h in ref.history if h["kind"] == "block"]
    first = next((i for i, (a, b) in enumerate(zip(blocks, ref_blocks)) if a["accept_rate"] != b["accept_rate"]), None)
    s, acc = follow_up(tgt, r, t.seed + 45)
    base = nuts_baseline(tgt, t, start)
    print("ratio %s step size %.4f (oracle %.4f) first block off the oracle's rate: %s | follow-up: acceptance %.4f rhat %.4f ess %.0f | HMC_NUTS: rhat %.3f ess %.1f"
          % (ratio, r.step_size, ref.step_size, first, acc, s.max_rhat(), s.min_ess(), base.max_rhat(), base.min_ess()))
    assert np.all((ratio >= 0.8) & (ratio <= 1.25)), ratio
    assert abs(r.step_size - ref.step_size) <= 0.10 * ref.step_size
    assert np.all(np.abs(r.inv_mass.cpu().numpy() - ref.inv_mass) <= 0.05 * ref.inv_mass)
    assert 0.65 <= acc <= 0.9
    assert s.max_rhat() <= 1.05
    assert s.min_ess() >= 10 * base.min_ess()


def test_warmup_on_a_compiled_closure():
    """log p = -sum log cosh(theta / s), s = (0.2, 1, 5), float32: an opaque callable, compiled into the trajectory kernel."""
    t = A.SECH
    s_ = torch.tensor(t.scale, dtype=torch.float32, device=DEV)
    f = lambda th: -torch.log(torch.cosh(th / s_)).sum()                        # noqa: E731
    start = torch.from_numpy(A.start(t)).to(DEV)
    r = ht.warmup(f, start, num_steps_per_sample=A.L, step_size=t.eps0, seed=t.seed)
    assert "hta_cb_hmc_kernel" in _abi.last_route(), _abi.last_route()
    ratio = r.inv_mass.double().cpu().numpy() / t.variance
    s, acc = follow_up(f, r, t.seed + 45)
    base = nuts_baseline(f, t, start)
    print("ratio %s step size %.4f | follow-up: acceptance %.4f rhat %.4f ess %.0f | HMC_NUTS: rhat %.3f ess %.1f"
          % (ratio, r.step_size, acc, s.max_rhat(), s.min_ess(), base.max_rhat(), base.min_ess()))
    assert np.all((ratio >= 0.75) & (ratio <= 1.3)), ratio
    assert 0.65 <= acc <= 0.92
    assert s.max_rhat() <= 1.05
    assert s.min_ess() >= 4 * base.min_ess()


def test_one_chain_and_host_starts():
    """a (D,) start is one chain: (D,) params back; a (C, D) start on the host: everything back on the host."""
    sd = torch.tensor([0.5, 2.0, 1.0])
    tgt = ht.GaussianTarget(torch.zeros(3, device=DEV), precision=torch.diag(1.0 / (sd * sd)).to(DEV))
    kw = dict(num_steps_per_sample=5, step_size=0.05, seed=3, block=5, windows=(2, 2), settle=1)
    one = ht.warmup(tgt, torch.zeros(3, device=DEV), **kw)
    assert one.params.shape == (3,) and one.params.is_cuda and one.inv_mass.shape == (3,) and one.step_size > 0
    assert len([h for h in one.history if h["kind"] == "block"]) == 5
    host = ht.warmup(ht.GaussianTarget(torch.zeros(3), precision=torch.diag(1.0 / (sd * sd))), torch.zeros(16, 3), **kw)
    assert host.params.shape == (16, 3) and not host.params.is_cuda and not host.inv_mass.is_cuda and host.inv_mass.shape == (3,)
    assert all(not v.is_cuda for h in host.history for v in h.values() if torch.is_tensor(v))
    assert bool(torch.isfinite(host.inv_mass).all()) and bool((host.inv_mass > 0).all())
    plain = ht.warmup(tgt, torch.zeros(16, 3, device=DEV), adapt_mass=False, **kw)
    assert plain.inv_mass is None and not [h for h in plain.history if h["kind"] == "window"]


def test_rmhmc_is_refused():
    tgt = ht.GaussianTarget(torch.zeros(3, device=DEV), precision=torch.eye(3, device=DEV))
    with pytest.raises(ValueError, match="RMHMC"):
        ht.warmup(tgt, torch.zeros(8, 3, device=DEV), sampler=ht.Sampler.RMHMC)


def test_a_refused_mass_on_the_device_keeps_the_previous_one():
    """Controller.observe_window with device tensors: checked and replaced without a read-back."""
    ctl = adapt.Controller(0.1, block=1, windows=(1, 1, 1), settle=0)
    good = torch.tensor([1.0, 2.0], device=DEV)
    masses = [torch.tensor([1.0, float("nan")], device=DEV), good, torch.tensor([0.0, 1.0], device=DEV)]
    seen = []
    for m in masses:
        ctl.next_block()
        ctl.observe_block(0.8)
        ctl.observe_window(m)
        seen.append(ctl.inv_mass.clone())
    assert torch.equal(seen[0], torch.ones(2, device=DEV)) and torch.equal(seen[1], good) and torch.equal(seen[2], good)
    assert [bool(h["accepted"]) for h in ctl.history if h["kind"] == "window"] == [False, True, False]


def test_warmup_with_around_sample_model():
    """Plumbing: the 8-100-1 MLP at 64 chains, a short schedule through a lambda around sample_model; the mass it returns goes
    back into sample_model on the native MLP route.  No mixing claim."""
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(8, 100), torch.nn.ReLU(), torch.nn.Linear(100, 1)).to(DEV)
    g = torch.Generator().manual_seed(0)
    X = torch.randn(400, 8, generator=g)
    Y = torch.sin(X @ torch.randn(8, 1, generator=g)) + 0.1 * torch.randn(400, 1, generator=g)
    X, Y = X.to(DEV), Y.to(DEV)
    D = 1001
    theta0 = (ht.util.flatten(net).detach() + 0.01 * torch.randn(64, D, generator=g).to(DEV)).contiguous()
    kw = dict(model_loss="regression", num_steps_per_sample=10, tau_out=100.0, tau_list=torch.ones(4), verbose=False)

    def run_block(params, n, eps, inv_mass, k):
        return ht.sample_model(net, X, Y, params, num_samples=n, step_size=eps, inv_mass=inv_mass, debug=2, seed=11 + k, **kw)

    r = adapt.warmup_with(run_block, theta0, adapt.Controller(5e-4, block=5, windows=(2, 2), settle=1))
    route = _abi.last_route()
    assert route.startswith(("mlp_mfma_kernel", "mlp1_hmc_kernel")), route
    assert r.inv_mass.shape == (D,) and r.inv_mass.dtype == torch.float32
    assert bool(torch.isfinite(r.inv_mass).all()) and bool((r.inv_mass > 0).all()) and math.isfinite(r.step_size) and r.step_size > 0
    out = ht.sample_model(net, X, Y, r.params, num_samples=6, step_size=r.step_size, inv_mass=r.inv_mass, seed=40, **kw)
    route = _abi.last_route()
    assert route.startswith(("mlp_mfma_kernel", "mlp1_hmc_kernel")), route
    assert torch.isfinite(torch.stack(list(out))).all()
