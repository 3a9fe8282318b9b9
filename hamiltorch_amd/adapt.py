"""Cross-chain warm-up: one step size and a diagonal or dense mass for a batch of chains, from block-wise acceptance rates and
the running moments (or, for the dense mass, the running covariance) of the chains' own draws.

    r = hamiltorch_amd.warmup(log_prob, start, num_steps_per_sample=10, step_size=0.01, seed=1)
    out = hamiltorch_amd.sample(log_prob, r.params, step_size=r.step_size, inv_mass=r.inv_mass, num_samples=1000, ...)

The schedule (`Controller`): trajectories run in BLOCKS of `block` at one step size; after a block the dual averaging of
`Sampler.HMC_NUTS` (samplers._dual_average) takes the block's acceptance rate, averaged over chains - one host read per block
instead of one per trajectory.  Blocks form PHASES: the `windows`, each a number of blocks whose draws go into a fresh
`diagnostics.RunningMoments`; at a window's end the mass becomes the regularised variance of those draws pooled over all chains
(with C chains a window of a few dozen trajectories holds thousands of draws per coordinate), computed and kept on the device.
A last phase of `settle` blocks tunes the step size for the final mass; its averaged iterate `eps_bar` is the result.

A phase after the first restarts the dual averaging (H_t = 0, eps_bar = 1) around the step size carried over from the phase
before: the first block runs at `carried` and the shrink point is log(carried), not the reference's log(10 eps) - after a mass
update that point sends the first block to a step size ten times too long, acceptance 0, and the few blocks of a phase do not
recover from it.

`mass="dense"` (Controller, warmup): the windows' draws go into a `diagnostics.RunningCovariance` and the mass becomes their
regularised pooled covariance, a (D, D) matrix - for targets whose badly scaled axes are not the coordinate axes.  With it the
target is close to a unit Gaussian in the mass's coordinates, where L leapfrog steps of size eps turn every coordinate by the
same angle L * 2 asin(eps / 2).  Near a multiple of pi the trajectory ends where it began (or at its mirror image) and the
chain stops mixing however good the mass is: at eps = 1.17 and L = 10 the angle is 3.98 pi.  Choose L for the runs after a
dense warm-up with that angle in mind - a short trajectory (L = 2 or 3) is usually right once the mass is dense.

`Controller` is plain Python (no device, no library): `warmup_with` drives it with any `run_block` - a lambda around
`sample_model`, or the CPU oracle in tests/test_adapt_cpu.py; `warmup` is `warmup_with` around `sample()`.
"""
from __future__ import annotations

from collections import namedtuple

Block = namedtuple("Block", "n_trajectories step_size inv_mass seed_index collect")
WarmupResult = namedtuple("WarmupResult", "params step_size inv_mass history")


def _mass_check(inv_mass, previous):
    """(mass to use, accepted) for a window's new inv_mass: a (D,) mass is refused when an entry is not finite or not positive,
    a (D, D) mass when an entry is not finite or the matrix is not positive definite (its Cholesky factorisation fails); the
    mass kept instead is `previous`, for a matrix without one the identity.  A device tensor is checked and replaced on the
    device (`accepted` is then a 0-d bool tensor: nothing is read back); anything else on the host."""
    dense = getattr(inv_mass, "ndim", 1) == 2
    if getattr(inv_mass, "is_cuda", False):
        import torch
        if dense:
            eye = torch.eye(inv_mass.shape[0], dtype=inv_mass.dtype, device=inv_mass.device)
            finite = torch.isfinite(inv_mass).all()
            ok = finite & (torch.linalg.cholesky_ex(torch.where(finite, inv_mass, eye)).info == 0)
            return torch.where(ok, inv_mass, eye if previous is None else previous), ok
        ok = (torch.isfinite(inv_mass) & (inv_mass > 0)).all()
        keep = torch.ones_like(inv_mass) if previous is None else previous
        return torch.where(ok, inv_mass, keep), ok
    import numpy as np
    v = np.asarray(inv_mass.detach().cpu() if hasattr(inv_mass, "detach") else inv_mass, dtype=np.float64)
    if dense:
        ok = bool(v.size) and v.shape[0] == v.shape[1] and bool(np.all(np.isfinite(v)))
        if ok:
            try:
                np.linalg.cholesky(v)
            except np.linalg.LinAlgError:
                ok = False
        if ok or previous is not None:
            return (inv_mass if ok else previous), ok
        if hasattr(inv_mass, "detach"):
            import torch
            return torch.eye(v.shape[0], dtype=inv_mass.dtype), ok
        return np.eye(v.shape[0], dtype=getattr(inv_mass, "dtype", np.float64)), ok
    ok = bool(v.size) and bool(np.all(np.isfinite(v) & (v > 0)))
    return (inv_mass if ok else previous), ok


class Controller:
    """The warm-up schedule as a state machine: `next_block()` -> Block(n_trajectories, step_size, inv_mass, seed_index,
    collect) or None at the end; run it; `observe_block(accept_rate)` with the block's acceptance rate averaged over chains;
    when `window_due` is set, `observe_window(inv_mass)` with the regularised pooled variance of the window's collected draws
    before the next block.  `seed_index` counts the blocks 0, 1, 2, ...: a block is a sampling call of its own and needs its
    own random stream.  `mass`: "diag" - observe_window takes a (D,) variance - or "dense" - a (D, D) covariance.
    `step_size` / `inv_mass`: the current values - after the last block the result.  `history`: one dict
    per block (kind="block", phase, index, step_size, accept_rate, eps_bar) and per window (kind="window", phase, accepted,
    whatever observe_window was told)."""

    def __init__(self, step_size, block=10, windows=(5, 5, 10, 20), settle=5, desired_accept_rate=0.8, adapt_mass=True,
                 reg_n=5, reg_floor=1e-3, mass="diag"):
        if mass not in ("diag", "dense"):
            raise ValueError("adapt.Controller: mass=%r; \"diag\" or \"dense\"" % (mass,))
        self.mass = mass
        self.block, self.windows, self.settle = int(block), tuple(int(w) for w in windows), int(settle)
        if not float(step_size) > 0.0:
            raise ValueError("adapt.Controller: step_size=%r" % (step_size,))
        if self.block < 1 or self.settle < 0 or any(w < 1 for w in self.windows) or not (self.windows or self.settle):
            raise ValueError("adapt.Controller: block=%r windows=%r settle=%r" % (block, windows, settle))
        if not 0.0 < float(desired_accept_rate) < 1.0:
            raise ValueError("adapt.Controller: desired_accept_rate=%r" % (desired_accept_rate,))
        self.desired, self.adapt_mass = float(desired_accept_rate), bool(adapt_mass)
        self.reg_n, self.reg_floor = reg_n, reg_floor
        #: (blocks, is a window) per phase
        self.phases = [(w, True) for w in self.windows] + ([(self.settle, False)] if self.settle else [])
        self.phase, self.index, self.seed_index = 0, 0, 0
        self.step_size, self.inv_mass = float(step_size), None
        self._init, self._H, self._eps_bar = float(step_size), 0.0, 1.0
        self.window_due, self._running = False, False
        self.history = []

    @property
    def done(self):
        return self.phase >= len(self.phases)

    @property
    def n_trajectories(self):
        """Trajectories of the whole schedule."""
        return self.block * sum(n for n, _ in self.phases)

    def next_block(self):
        if self._running:
            raise RuntimeError("adapt.Controller: observe_block() of the running block first")
        if self.window_due:
            raise RuntimeError("adapt.Controller: observe_window() of the finished window first")
        if self.done:
            return None
        self._running = True
        return Block(self.block, self.step_size, self.inv_mass, self.seed_index, self.adapt_mass and self.phases[self.phase][1])

    def observe_block(self, accept_rate):
        if not self._running:
            raise RuntimeError("adapt.Controller: no block is running")
        from .samplers import _dual_average
        alpha = float(accept_rate)
        if not alpha == alpha:                                      # a NaN rate: every trajectory counted as rejected
            alpha = 0.0
        used = self.step_size
        eps, self._eps_bar, self._H = _dual_average(min(1.0, max(0.0, alpha)), self.index, self._init, self._H, self._eps_bar, self.desired)
        self.history.append(dict(kind="block", phase=self.phase, index=self.index, seed_index=self.seed_index, step_size=used,
                                 accept_rate=alpha, eps_bar=self._eps_bar))
        self._running = False
        self.seed_index += 1
        self.index += 1
        self.step_size = eps
        if self.index == self.phases[self.phase][0]:                # the phase ends: restart around its averaged iterate
            carried = self._eps_bar
            self.window_due = self.adapt_mass and self.phases[self.phase][1]
            self.phase, self.index = self.phase + 1, 0
            self.step_size, self._init, self._H, self._eps_bar = carried, carried / 10.0, 0.0, 1.0

    def observe_window(self, inv_mass, **record):
        if not self.window_due:
            raise RuntimeError("adapt.Controller: no window has just ended")
        if getattr(inv_mass, "ndim", None) != (2 if self.mass == "dense" else 1):
            raise ValueError("adapt.Controller: mass=%r takes a %s inv_mass" % (self.mass, "(D, D)" if self.mass == "dense" else "(D,)"))
        self.inv_mass, ok = _mass_check(inv_mass, self.inv_mass)
        self.history.append(dict(kind="window", phase=self.phase - 1, accepted=ok, **record))
        self.window_due = False


def _mean_rate(rate):
    """The block's acceptance rate over chains as a float: THE host read of a block."""
    if hasattr(rate, "double"):
        return float(rate.double().mean())
    import numpy as np
    return float(np.mean(np.asarray(rate, dtype=np.float64)))


def warmup_with(run_block, params_init, controller, moments_factory=None):
    """Drive `controller` with `run_block(params[C, D], n, step_size, inv_mass, seed_index)` -> (rows, accept_rate[C]): rows as
    sample() returns them - rows[0] is `params`, rows[1:] the block's draws, rows[-1] the next block's start.  The draws of a
    window go into a fresh `moments_factory()` (default diagnostics.RunningMoments, under controller.mass == "dense"
    diagnostics.RunningCovariance; anything with update(rows, skip) and result(reg_n, reg_floor, dtype) -> .inv_mass, .sd,
    .rhat, .n_draws), whose regularised pooled variance - or covariance - becomes the mass.
    Returns WarmupResult(params, step_size, inv_mass, history)."""
    if moments_factory is None:
        if controller.mass == "dense":
            from .diagnostics import RunningCovariance as moments_factory
        else:
            from .diagnostics import RunningMoments as moments_factory
    params, acc = params_init, None
    while True:
        blk = controller.next_block()
        if blk is None:
            break
        rows, rate = run_block(params, blk.n_trajectories, blk.step_size, blk.inv_mass, blk.seed_index)
        if blk.collect:
            if acc is None:
                acc = moments_factory()
            acc.update(rows, skip=1)
        params = rows[-1]
        controller.observe_block(_mean_rate(rate))
        if controller.window_due:
            res = acc.result(reg_n=controller.reg_n, reg_floor=controller.reg_floor, dtype=getattr(params, "dtype", None))
            controller.observe_window(res.inv_mass, n_draws=res.n_draws, sd=res.sd, rhat=res.rhat)
            acc = None
    return WarmupResult(params, controller.step_size, controller.inv_mass, controller.history)


def warmup(log_prob_func, params_init, num_steps_per_sample=10, step_size=0.1, *, seed=None, chain_offset=0, block=10,
           windows=(5, 5, 10, 20), settle=5, desired_accept_rate=0.8, adapt_mass=True, reg_n=5, reg_floor=1e-3, mass="diag",
           **sample_kwargs):
    """Warm-up of `sample(log_prob_func, params_init, ...)` with Sampler.HMC (any of its integrators; a list of callables under
    the split ones): block k is sample(..., num_samples=block, burn=0, seed=seed + k) from where block k - 1 ended.  A (D,)
    `params_init` is one chain; a start on the host is staged once and the result comes back on the host.  `sample_kwargs`:
    further arguments of sample() (integrator, native, pass_grad, ...).  Returns WarmupResult(params, step_size, inv_mass,
    history) for

        sample(log_prob_func, r.params, step_size=r.step_size, inv_mass=r.inv_mass, ...)

    `mass="diag"`: inv_mass is the (D,) pooled variance; one host read per block (its acceptance rate), none per window.
    `mass="dense"`: inv_mass is the (D, D) pooled covariance from diagnostics.RunningCovariance (D <= COVARIANCE_MAX_D); the
    window's matrix is checked on the device without a read-back, but every block's sample() call inverts and factors the
    matrix through torch, and those calls read a status back - the one-read-per-block statement holds for "diag" only.  After
    a dense warm-up the target is close to a unit Gaussian in the mass's coordinates and a trajectory turns every coordinate
    by the same angle L * 2 asin(step_size / 2): pick L for the runs that follow so that this angle stays away from
    multiples of pi, or the chains return to where they started (the module docstring)."""
    import torch
    from . import util
    from .enums import Sampler
    from .samplers import sample
    sampler = sample_kwargs.pop("sampler", Sampler.HMC)
    if sampler != Sampler.HMC:
        raise ValueError("adapt.warmup: sampler=%s; the warm-up adapts the step size and the mass of Sampler.HMC - RMHMC takes its "
                         "metric from the target's curvature and HMC_NUTS adapts a step size of its own in its burn-in" % (sampler,))
    if mass not in ("diag", "dense"):
        raise ValueError("adapt.warmup: mass=%r; \"diag\" or \"dense\"" % (mass,))
    for k in ("num_samples", "burn", "inv_mass", "debug", "verbose", "store_on_GPU"):
        if k in sample_kwargs:
            raise ValueError("adapt.warmup: %s is set by the warm-up itself" % k)
    if not torch.is_tensor(params_init) or params_init.dim() not in (1, 2):
        raise ValueError("adapt.warmup: params_init must be a (D,) or (C, D) tensor")
    one, host = params_init.dim() == 1, not params_init.is_cuda
    if mass == "dense":
        from .diagnostics import COVARIANCE_MAX_D
        if params_init.shape[-1] > COVARIANCE_MAX_D:
            raise ValueError("adapt.warmup: mass=\"dense\" keeps D (D + 1) / 2 co-moments per chain and is limited to D <= %d; D=%d"
                             % (COVARIANCE_MAX_D, params_init.shape[-1]))
    theta = params_init.detach().reshape(1, -1) if one else params_init.detach()
    if host:
        from .host import _device, lift_callable
        theta = theta.to(_device())
        log_prob_func = lift_callable(log_prob_func, theta)
    seed = util.next_stream_seed() if seed is None else int(seed)
    ctl = Controller(step_size, block, windows, settle, desired_accept_rate, adapt_mass, reg_n, reg_floor, mass=mass)

    def run_block(params, n, eps, inv_mass, k):
        return sample(log_prob_func, params, num_samples=n, num_steps_per_sample=num_steps_per_sample, step_size=eps, burn=0,
                      inv_mass=inv_mass, sampler=Sampler.HMC, debug=2, verbose=False, seed=seed + k, chain_offset=chain_offset,
                      **sample_kwargs)

    r = warmup_with(run_block, theta, ctl)
    params, inv_mass, history = r.params, r.inv_mass, r.history
    if one:
        params = params.reshape(-1)
    if host:
        params = params.cpu()
        inv_mass = None if inv_mass is None else inv_mass.cpu()
        history = [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in h.items()} for h in history]
    return WarmupResult(params, r.step_size, inv_mass, history)
