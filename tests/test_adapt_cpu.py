"""CPU: the warm-up's schedule (adapt.Controller) against schedules computed by hand from the oracle's dual averaging, and
adapt.warmup_with driven by the CPU oracle on the two targets of tests/adapt_cases.py, held to the conditions the GPU test
(tests/test_gpu_adapt.py) puts on the engines - so the reference side of that test stays inside them on its own."""
import numpy as np
import pytest

import adapt_cases as A
import hmc_oracle as O
from hamiltorch_amd import adapt


def drive(ctl, rates, masses=()):
    """Run the controller over the acceptance rates -> the blocks it handed out."""
    blocks, masses = [], list(masses)
    for a in rates:
        blocks.append(ctl.next_block())
        ctl.observe_block(a)
        if ctl.window_due:
            ctl.observe_window(masses.pop(0))
    return blocks


def test_the_schedule_by_hand():
    """block = 2, windows (2, 1), settle 2, from step size 0.1: block and phase order, the seed indices, the step size of every
    block and the restart of a phase around the step size it inherits."""
    ctl = adapt.Controller(0.1, block=2, windows=(2, 1), settle=2)
    assert ctl.n_trajectories == 10 and not ctl.done and ctl.inv_mass is None
    rates = [0.95, 0.6, 0.9, 0.7, 0.85]
    m1, m2 = np.array([1.0, 4.0]), np.array([2.0, 3.0])
    blocks = drive(ctl, rates, [m1, m2])
    assert ctl.done and ctl.next_block() is None
    # phase 0: the reference's schedule around step_size
    e1, b1, h1 = O.dual_average(0.95, 0, 0.1, 0.0, 1.0, 0.8)
    e2, b2, h2 = O.dual_average(0.6, 1, 0.1, h1, b1, 0.8)
    # phase 1 starts at b2 with H_t = 0, eps_bar = 1 and the shrink point log(b2); phase 2 at that phase's eps_bar
    e3, b3, h3 = O.dual_average(0.9, 0, b2 / 10.0, 0.0, 1.0, 0.8)
    e4, b4, h4 = O.dual_average(0.7, 0, b3 / 10.0, 0.0, 1.0, 0.8)
    e5, b5, h5 = O.dual_average(0.85, 1, b3 / 10.0, h4, b4, 0.8)
    assert [b.step_size for b in blocks] == [0.1, e1, b2, b3, e4]
    assert [b.seed_index for b in blocks] == [0, 1, 2, 3, 4]
    assert [b.n_trajectories for b in blocks] == [2] * 5
    assert [b.collect for b in blocks] == [True, True, True, False, False]
    assert blocks[0].inv_mass is None and blocks[1].inv_mass is None and blocks[2].inv_mass is m1 and blocks[3].inv_mass is m2 and blocks[4].inv_mass is m2
    assert ctl.step_size == b5 and ctl.inv_mass is m2
    recs = [h for h in ctl.history if h["kind"] == "block"]
    assert [(h["phase"], h["index"]) for h in recs] == [(0, 0), (0, 1), (1, 0), (2, 0), (2, 1)]
    assert [h["eps_bar"] for h in recs] == [b1, b2, b3, b4, b5] and [h["accept_rate"] for h in recs] == rates
    assert [h["step_size"] for h in recs] == [b.step_size for b in blocks]
    assert [(h["phase"], h["accepted"]) for h in ctl.history if h["kind"] == "window"] == [(0, True), (1, True)]


def test_a_restarted_phase_shrinks_towards_the_step_size_it_inherits():
    """a block at the desired rate right after a restart leaves the step size where it was (the reference's shrink point
    log(10 eps) would move it up tenfold); the first block of the first phase does go to 10 eps - the reference's schedule."""
    ctl = adapt.Controller(0.3, block=3, windows=(1,), settle=2, adapt_mass=False)
    assert ctl.next_block().collect is False                   # no mass adaptation: nothing to collect
    ctl.observe_block(0.8)
    assert not ctl.window_due
    carried = ctl.step_size
    assert ctl.history[-1]["eps_bar"] == carried
    assert ctl.next_block().step_size == carried
    ctl.observe_block(0.8)
    assert ctl.step_size == pytest.approx(carried, rel=1e-6)
    first = adapt.Controller(0.3, windows=(2,), settle=0)
    first.next_block()
    first.observe_block(0.8)
    assert first.step_size == pytest.approx(3.0, rel=1e-6)


def test_a_bad_mass_is_refused():
    ctl = adapt.Controller(0.1, block=1, windows=(1, 1, 1, 1), settle=1)
    good = np.array([1.0, 2.0])
    blocks = drive(ctl, [0.8] * 5, [np.array([1.0, np.nan]), good, np.array([0.0, 1.0]), np.array([np.inf, 1.0])])
    assert [b.inv_mass is None for b in blocks] == [True, True, False, False, False]
    assert blocks[2].inv_mass is good and blocks[4].inv_mass is good and ctl.inv_mass is good
    assert [h["accepted"] for h in ctl.history if h["kind"] == "window"] == [False, True, False, False]


def test_the_calls_come_in_order():
    ctl = adapt.Controller(0.1, block=1, windows=(1,), settle=1)
    with pytest.raises(RuntimeError, match="no block is running"):
        ctl.observe_block(0.8)
    with pytest.raises(RuntimeError, match="no window"):
        ctl.observe_window(np.ones(2))
    ctl.next_block()
    with pytest.raises(RuntimeError, match="observe_block"):
        ctl.next_block()
    ctl.observe_block(0.8)
    with pytest.raises(RuntimeError, match="observe_window"):
        ctl.next_block()
    for bad in (dict(step_size=0.0), dict(step_size=0.1, block=0), dict(step_size=0.1, windows=(), settle=0), dict(step_size=0.1, windows=(0,)),
                dict(step_size=0.1, desired_accept_rate=1.0)):
        with pytest.raises(ValueError):
            adapt.Controller(**bad)


def test_warmup_refuses_what_it_cannot_adapt():
    """before anything touches a device: the samplers without a step size / mass of this kind, and the arguments it sets itself."""
    import torch
    import hamiltorch_amd as ht
    assert ht.warmup is adapt.warmup and ht.adapt is adapt
    f = lambda th: -(th * th).sum()                                # noqa: E731
    for s in (ht.Sampler.RMHMC, ht.Sampler.HMC_NUTS):
        with pytest.raises(ValueError, match="Sampler.HMC"):
            ht.warmup(f, torch.zeros(3), sampler=s)
    with pytest.raises(ValueError, match="set by the warm-up"):
        ht.warmup(f, torch.zeros(3), burn=3)
    with pytest.raises(ValueError, match="params_init"):
        ht.warmup(f, torch.zeros(2, 3, 4))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_oracle_driven_warmup_on_the_anisotropic_gaussian(dtype):
    """sd = (0.05, 0.5, 1, 5) from eps0 = 0.01: the conditions of the GPU test on the oracle's own run."""
    t = A.GAUSS
    r, ctl = A.oracle_warmup(t, dtype)
    ratio = np.asarray(r.inv_mass, dtype=np.float64) / t.variance
    x, acc = A.oracle_follow_up(t, r, ctl.seed_index, dtype)
    rhat, ess = A.diagnostics(x)
    xn, eps_nuts = A.oracle_nuts(t, dtype)
    rhat_nuts, ess_nuts = A.diagnostics(xn)
    print("ratio %s step size %.4f acceptance %.4f rhat %.4f ess %.0f | HMC_NUTS: step size %.4f rhat %.3f ess %.1f"
          % (ratio, r.step_size, acc, rhat, ess, eps_nuts, rhat_nuts, ess_nuts))
    assert ctl.seed_index == 45 and len(ctl.history) == 45 + 4
    assert np.all((ratio >= 0.8) & (ratio <= 1.25)), ratio
    assert 0.65 <= acc <= 0.9
    assert rhat <= 1.05
    assert ess >= 10 * ess_nuts


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_oracle_driven_warmup_on_the_sech_product(dtype):
    """log p = -sum log cosh(theta / s), s = (0.2, 1, 5), from eps0 = 0.02."""
    t = A.SECH
    r, ctl = A.oracle_warmup(t, dtype)
    ratio = np.asarray(r.inv_mass, dtype=np.float64) / t.variance
    x, acc = A.oracle_follow_up(t, r, ctl.seed_index, dtype)
    rhat, ess = A.diagnostics(x)
    xn, eps_nuts = A.oracle_nuts(t, dtype)
    rhat_nuts, ess_nuts = A.diagnostics(xn)
    print("ratio %s step size %.4f acceptance %.4f rhat %.4f ess %.0f | HMC_NUTS: step size %.4f rhat %.3f ess %.1f"
          % (ratio, r.step_size, acc, rhat, ess, eps_nuts, rhat_nuts, ess_nuts))
    assert np.all((ratio >= 0.75) & (ratio <= 1.3)), ratio
    assert 0.65 <= acc <= 0.92
    assert rhat <= 1.05
    assert ess >= 4 * ess_nuts


def test_the_history_of_a_warmup():
    """one record per block and per window; a window's record carries its draws (9 per block and chain), pooled sd and R-hat."""
    r, ctl = A.oracle_warmup(A.GAUSS, np.float32, block=10, windows=(2, 3), settle=1)
    blocks = [h for h in r.history if h["kind"] == "block"]
    wins = [h for h in r.history if h["kind"] == "window"]
    assert len(blocks) == 6 and [h["n_draws"] for h in wins] == [18, 27] and all(h["accepted"] for h in wins)
    assert wins[0]["sd"].shape == (4,) and wins[0]["rhat"].shape == (4,)
    assert r.step_size == blocks[-1]["eps_bar"] and r.params.shape == (A.CHAINS, 4) and r.inv_mass.dtype == np.float32
