"""Callback compiler: an OPAQUE ``log_prob_func`` inside fused gfx950 kernels.

The reference's hot spot for a general target is ``params_grad`` (hamiltorch/samplers.py:270-278 -> ``collect_gradients``
:33-66): autograd through the user's callable, once per leapfrog step - "84 % of HMC wall time" on its own CPU path, and on a
GPU ~38 eager launches per step around kernels that take microseconds.  This package removes the launches:

  roll.py     a likelihood summed over many data rows - too large as straight-line code - is ROLLED: one term function, a table
              of per-row constants, a loop split over the waves of a workgroup (``csrc/jit/rolled_callback.hip.in``);
  trace.py    the callable is traced ONCE per target (torch.fx ``make_fx``) and lowered element by element to a scalar graph;
  ir.py       reverse-mode differentiation, simplification and common-subexpression sharing on that graph;
  emit.py     value + gradient (and, for the Riemannian samplers, Hessian + third-derivative contraction) as straight-line
              HIP device code;
  runtime.py  hipRTC (through the C ABI: ``hta_jit_compile`` / ``hta_jit_load``) builds that text INTO the hand-written
              kernels of ``csrc/jit/`` - for plain HMC the whole ``sample()`` loop, one chain per lane, one launch per block
              of trajectories; for the split integrators (``log_prob_func`` is a LIST of callables, one per data subset) the
              same loop around all of them: ``compile_split``, ``csrc/jit/split_callback.hip.in``; for ``leapfrog()`` on a
              batch of chains the per-step path of either: ``compile_path``, ``csrc/jit/path_callback.hip.in``.

No inductor, no Triton, no code from torch's compiler stack beyond the tracer.  A callable the tracer or the lowering table
does not cover (data-dependent control flow, the tuple / ``pass_grad`` protocols, unlisted operations, graphs that are too
large) stays on the torch-evaluated callback path; ``last_reason()`` and ``hta_last_route()`` say why.  Every compiled run is
checked against the callable itself on the states it ended in (``samplers._verify_compiled``); a mismatch re-traces once and
otherwise repeats the run on the callback path.  ``HAMILTORCH_AMD_JIT=0`` (or ``sample(..., native=False)``) turns it off.
"""
from __future__ import annotations

import os
import threading
import weakref

import torch

from . import runtime
from .ir import Unsupported
from .trace import trace_callback

_lock = threading.Lock()
_by_fn = weakref.WeakKeyDictionary()      # callable -> {config: entry}
_state = threading.local()
stats = {"traced": 0, "trace_hits": 0, "unsupported": 0}


def enabled():
    return os.environ.get("HAMILTORCH_AMD_JIT", "1") != "0"


def last_reason():
    """Why the calling thread's last compile attempt fell back to the callback path ('' if it did not)."""
    return getattr(_state, "reason", "")


def _note(reason):
    _state.reason = reason


def _signature(fn):
    """Identity + version counters of what `fn` closes over and of the tensors / objects its code names in its globals: the key
    under which a trace is reused.  Holds the objects (their ids stay unique while the entry lives).  In-place changes deeper
    inside captured objects are NOT seen here - the run-time check against the callable catches those."""
    objs = []
    f = getattr(fn, "__func__", fn)
    if getattr(fn, "__self__", None) is not None:
        objs.append(fn.__self__)
    for cell in (getattr(f, "__closure__", None) or ()):
        try:
            objs.append(cell.cell_contents)
        except ValueError:
            objs.append(None)
    code, glob = getattr(f, "__code__", None), getattr(f, "__globals__", None)
    if code is not None and glob is not None:
        for name in code.co_names:
            v = glob.get(name)
            if torch.is_tensor(v) or isinstance(v, (torch.distributions.Distribution, torch.nn.Module)):
                objs.append(v)
    if isinstance(fn, torch.nn.Module):
        objs += list(fn.parameters()) + list(fn.buffers())
    for a in (getattr(fn, "args", None) or ()) if hasattr(fn, "func") else ():      # functools.partial
        objs.append(a)
    sig = tuple((id(o), getattr(o, "_version", None), float(o) if isinstance(o, (int, float)) and not isinstance(o, bool) else None)
                for o in objs)
    return sig, objs


class CompiledPath:
    """A traced callable, or a list of them, compiled into the leapfrog-path kernel (csrc/jit/path_callback.hip.in) for one
    (D, dtype, mass kind); `M` is the length of the list, 0 for a single callable."""

    def __init__(self, traced, key, blob, dtype, mass_kind):
        self.traced, self.key, self.blob, self.dtype, self.mass_kind = traced, key, blob, dtype, mass_kind

    @property
    def M(self):
        return len(self.traced) if isinstance(self.traced, list) else 0

    def module(self, device):
        return runtime.module_for(self.key, self.blob, device)


class CompiledHMC:
    """A traced callable compiled into the HMC trajectory kernel for one (D, dtype, mass kind).  The generated text is kept; the
    code objects around it are built when first asked for - `key` / `blob`: the trajectory kernel's (at once by compile_hmc and
    its siblings), `path()`: the leapfrog-path kernel's (compile_path) - so that a trace made for one serves the other."""

    def __init__(self, traced, generated, skeleton, dtype, mass_kind):
        self.traced, self.generated, self.skeleton, self.dtype, self.mass_kind = traced, generated, skeleton, dtype, mass_kind
        self._code = self._path = None

    def _built(self):
        if self._code is None:
            self._code = runtime.compile_source(self.generated, self.skeleton)
        return self._code

    @property
    def key(self):
        return self._built()[0]

    @property
    def blob(self):
        return self._built()[1]

    def module(self, device):
        return runtime.module_for(self.key, self.blob, device)

    def path(self):
        if self.skeleton not in (runtime.SKELETON_HMC, runtime.SKELETON_SPLIT):
            raise Unsupported("leapfrog paths are compiled for plain HMC and the split integrators only")
        if self._path is None:
            key, blob = runtime.compile_source(self.generated, runtime.SKELETON_PATH)
            self._path = CompiledPath(self.traced, key, blob, self.dtype, self.mass_kind)
        return self._path


class CompiledRolled(CompiledHMC):
    """A traced callable ROLLED over its data rows (roll.py) and compiled into the rolled trajectory kernel
    (csrc/jit/rolled_callback.hip.in).  The generated text holds the term functions and no data: `rolled.groups[k].table` are the
    per-row constants an engine uploads, and callables of one structure over different data share one code object."""

    def __init__(self, traced, rolled, generated, dtype, mass_kind):
        super().__init__(traced, generated, runtime.SKELETON_ROLLED, dtype, mass_kind)
        self.rolled = rolled

    def path(self):
        raise Unsupported("a likelihood rolled over its %d data rows is compiled for sample() with plain HMC only, not for leapfrog() paths "
                          "(straight-line code for it is beyond %d scalar operations)" % (sum(self.rolled.rows), runtime.MAX_HMC_NODES))


class CompiledDerivs(CompiledHMC):
    """A traced callable compiled into the derivative kernels of the Riemannian samplers (csrc/jit/derivs_callback.hip.in) - or, with a
    generated include made for a metric, into the explicit-RMHMC trajectory kernel; `implicit()`: the implicit integrator's kernel
    around the SAME include (csrc/jit/rmhmc_implicit_callback.hip.in), a module of its own, built when first asked for."""

    _implicit = None

    def implicit(self):
        if self.skeleton != runtime.SKELETON_RMHMC:
            raise Unsupported("the implicit-RMHMC trajectory kernel is built around an RMHMC include only")
        if self._implicit is None:
            key, blob = runtime.compile_source(self.generated, runtime.SKELETON_RMHMC_IMPLICIT)
            self._implicit = CompiledPath(self.traced, key, blob, self.dtype, self.mass_kind)
        return self._implicit


def compile_hmc(fn, example, dtype, mass_kind, fresh=False):
    """CompiledHMC for ``fn`` at points shaped like the (D,) tensor ``example``; raises ``Unsupported``.  A trace is reused while the
    callable's closure signature is unchanged (``fresh=True`` traces again)."""
    return _compile(fn, example, dtype, int(mass_kind), fresh)


def compile_derivs(fn, example, dtype, fresh=False):
    """CompiledDerivs (value / gradient / Hessian + third-derivative contraction kernels) for ``fn``; raises ``Unsupported``."""
    return _compile(fn, example, dtype, "derivs", fresh)


# cache kinds of the explicit-RMHMC trajectory kernels -> (metric, jitter): the metric is part of the key, one entry (and one code object) each
_RMHMC_KINDS = {"rmhmc": ("softabs", False), "rmhmc-jitter": ("softabs", True), "rmhmc-hess": ("hessian", False), "rmhmc-hess-jitter": ("hessian", True)}


def compile_rmhmc(fn, example, dtype, jitter, fresh=False, metric="softabs", integrator="explicit"):
    """The callable built into the explicit-RMHMC trajectory kernel (csrc/jit/rmhmc_callback.hip.in; D <= 16) under `metric`
    ("softabs": rmhmc_metric_softabs.inc, "hessian": rmhmc_metric_hessian.inc); raises ``Unsupported``.  integrator="implicit": the
    implicit integrator's kernel (csrc/jit/rmhmc_implicit_callback.hip.in) around the same trace, checks and generated include - a
    callable already traced for one integrator is not traced again for the other, only the other module is built."""
    if (metric, bool(jitter)) not in _RMHMC_KINDS.values():
        raise ValueError("compile_rmhmc: metric is 'softabs' or 'hessian', got %r" % (metric,))
    if integrator not in ("explicit", "implicit"):
        raise ValueError("compile_rmhmc: integrator is 'explicit' or 'implicit', got %r" % (integrator,))
    if example.numel() > runtime.MAX_RMHMC_DIM:
        _note("D = %d: the chain-per-lane Riemannian kernel holds a chain's matrices in registers (D <= %d)" % (example.numel(), runtime.MAX_RMHMC_DIM))
        raise Unsupported(last_reason())
    kind = next(k for k, v in _RMHMC_KINDS.items() if v == (metric, bool(jitter)))
    return _compile(fn, example, dtype, kind, fresh, path="implicit" if integrator == "implicit" else False)


def compile_path(fn_or_list, example, dtype, mass_kind, fresh=False):
    """CompiledPath for a callable (plain HMC) or a list of callables (the split integrators) at points shaped like the (D,) tensor
    ``example``: what ``samplers.leapfrog`` runs a (C, D) batch of chains on; raises ``Unsupported``.  Traces go through the cache
    of ``compile_hmc`` / ``compile_split`` - a callable already traced for ``sample()`` is not traced again, only the path module
    is built (and a callable first seen here is not traced again by ``sample()``); every new trace is checked against
    torch.autograd like theirs."""
    if isinstance(fn_or_list, (list, tuple)):
        return compile_split(fn_or_list, example, dtype, mass_kind, fresh, _path=True)
    return _compile(fn_or_list, example, dtype, int(mass_kind), fresh, path=True)


def _finish(out, path):
    """Build the code object the caller asked for (the trajectory kernel's, the path kernel's, or - path = "implicit" - the
    implicit-RMHMC kernel's) around a compiled entry.  hipRTC turning
    the generated text down (an emitter bug, a device function hipRTC lacks) is not the user's problem: the callable runs on the
    previous path, the reason (the compiler's first error line) is reported like any other refusal."""
    try:
        if path == "implicit":
            return out.implicit()
        if path:
            return out.path()
        out._built()
        return out
    except runtime.CompileError as e:
        first = next((ln for ln in e.log.splitlines() if "error" in ln), str(e).splitlines()[0])
        raise Unsupported("hipRTC rejected the generated code: %s" % first.strip()[:160]) from None


def _compile(fn, example, dtype, mass_kind, fresh, path=False):
    _note("")
    # (the rolling switches are part of the key: an entry made under one setting is not handed out under another)
    # ('force' rolls for sample() what it keeps straight-line for leapfrog(): there the two callers do not share an entry)
    cfg = (int(example.numel()), dtype, mass_kind, example.device.type, runtime.roll_mode(), runtime.rolled_table_mode(),
           path is True and runtime.roll_mode() == "force")
    sig = objs = None
    try:
        sig, objs = _signature(fn)
        with _lock:
            ent = _by_fn.get(fn, {}).get(cfg)
    except TypeError:       # not weak-referenceable / unhashable: no reuse
        ent = None
        sig = None
    if ent is not None and not fresh and ent[0] == sig:
        stats["trace_hits"] += 1
        if isinstance(ent[2], Unsupported):
            _note(str(ent[2]))
            raise ent[2]
        return _hit(ent[2], path)
    try:
        traced = trace_callback(fn, example)
        stats["traced"] += 1
        if mass_kind == "derivs" or mass_kind in _RMHMC_KINDS:
            _too_large_unrolled(traced, runtime.MAX_DERIV_NODES, "the derivative and RMHMC kernels")
            _check_against_autograd(traced, fn, example)
            if mass_kind == "derivs":
                out = CompiledDerivs(traced, runtime.derivs_generated_source(traced, dtype), runtime.SKELETON_DERIVS, dtype, mass_kind)
            else:
                metric, jitter = _RMHMC_KINDS[mass_kind]
                out = CompiledDerivs(traced, runtime.derivs_generated_source(traced, dtype, jitter, metric), runtime.SKELETON_RMHMC, dtype, mass_kind)
        else:
            out = _hmc_or_rolled(traced, fn, example, dtype, mass_kind, path)
        try:
            ret = _finish(out, path)
        except Unsupported as e:
            if not isinstance(out, CompiledRolled):
                raise
            # a leapfrog() path was asked of a callable that compiles in its rolled form only: refused with that reason, and the
            # rolled entry is kept for sample()
            stats["unsupported"] += 1
            _note(str(e))
            ret = e
    except Unsupported as e:
        stats["unsupported"] += 1
        _note(str(e))
        out = e
    if sig is not None:
        try:
            with _lock:
                _by_fn.setdefault(fn, {})[cfg] = (sig, objs, out)
        except TypeError:
            pass
    if isinstance(out, Unsupported):
        raise out
    if isinstance(ret, Unsupported):
        raise ret
    return ret


def _too_large_unrolled(traced, limit, who):
    """A value graph that is beyond `limit` scalar operations on its own is refused BEFORE it is differentiated (the derivatives of
    an unrolled likelihood over thousands of rows take seconds to build, only to be turned down for their size)."""
    live = len(traced.graph.reachable([traced.value]))
    if live > limit:
        raise Unsupported("the value alone is %d scalar operations (limit %d with its derivatives); likelihoods rolled over their data rows "
                          "are compiled for a single callable under plain HMC in sample(), not for %s" % (live, limit, who))


def _hmc_or_rolled(traced, fn, example, dtype, mass_kind, path):
    """The straight-line trajectory kernel's entry for a traced callable - or, where HAMILTORCH_AMD_JIT_ROLL allows it, the rolled
    one (roll.py).  'auto' rolls only what the straight-line route refuses FOR ITS SIZE, and looks at the value graph's own size
    first so that the gradient of an unrolled likelihood is not built just to be thrown away; everything that compiled before keeps
    its text.  'force' rolls whenever a group exists (leapfrog() paths excepted: they have no rolled form)."""
    mode = runtime.roll_mode()
    big = len(traced.graph.reachable([traced.value])) > runtime.MAX_HMC_NODES
    if (mode == "auto" and big) or (mode == "force" and (big or not path)):
        try:
            return _rolled(traced, fn, example, dtype, mass_kind)
        except Unsupported as e:
            if big:
                raise Unsupported("the value is %d scalar operations (limit %d for straight-line code) and it does not roll: %s"
                                  % (len(traced.graph.reachable([traced.value])), runtime.MAX_HMC_NODES, e)) from None
            _note("not rolled: %s" % e)      # 'force' on a callable that fits straight-line code: that route, the reason kept until it compiles
    _check_against_autograd(traced, fn, example)
    try:
        return CompiledHMC(traced, runtime.hmc_generated_source(traced, dtype, mass_kind), runtime.SKELETON_HMC, dtype, mass_kind)
    except Unsupported as e:
        if mode != "auto" or "scalar operations (limit" not in str(e) or traced.D > runtime.MAX_HMC_DIM:
            raise
        try:
            return _rolled(traced, fn, example, dtype, mass_kind)
        except Unsupported as e2:
            raise Unsupported("%s and it does not roll: %s" % (e, e2)) from None


def _rolled(traced, fn, example, dtype, mass_kind):
    rolled = runtime.rolled_program(traced)
    _check_against_autograd(traced, fn, example, evaluate=lambda pts: rolled.evaluate(pts, "float64"))
    return CompiledRolled(traced, rolled, runtime.rolled_generated_source(rolled, dtype, mass_kind), dtype, mass_kind)


def _hit(out, path):
    """A cached entry for a caller that may want the other of its two code objects (built now, once)."""
    try:
        return _finish(out, path)
    except Unsupported as e:
        _note(str(e))
        raise


class CompiledSplit(CompiledHMC):
    """A LIST of traced callables (one per data subset) compiled into the split-HMC trajectory kernel
    (csrc/jit/split_callback.hip.in) for one (D, dtype, mass kind); `traced` is the list of traces, `M` its length."""

    @property
    def M(self):
        return len(self.traced)


def compile_split(fns, example, dtype, mass_kind, fresh=False, _path=False):
    """CompiledSplit for the list of callables ``fns`` (Integrator.SPLITTING / SPLITTING_RAND / SPLITTING_KMID: one callable per
    data subset) at points shaped like the (D,) tensor ``example``; raises ``Unsupported``.  Every callable is traced and checked
    against torch.autograd like a single one; one unsupported subset makes the whole list unsupported, and the reason names it.
    The result is reused while the tuple of the callables' closure signatures is unchanged (``fresh=True`` traces again)."""
    _note("")
    fns = list(fns)
    mass_kind = int(mass_kind)
    cfg = ("split", len(fns), int(example.numel()), dtype, mass_kind, example.device.type)
    sig = objs = refs = None
    ent = None
    try:
        if not fns or not all(callable(f) for f in fns):
            raise TypeError
        parts = [_signature(f) for f in fns]
        sig, objs = tuple(p[0] for p in parts), [p[1] for p in parts]
        refs = [weakref.ref(f) for f in fns[1:]]
        with _lock:
            ent = _by_fn.get(fns[0], {}).get(cfg)
    except TypeError:       # an empty list, or a member that is not weak-referenceable / hashable: no reuse
        ent = None
        sig = None
    if ent is not None and not fresh and ent[0] == sig and len(ent[3]) == len(fns) - 1 and all(r() is f for r, f in zip(ent[3], fns[1:])):
        stats["trace_hits"] += 1
        if isinstance(ent[2], Unsupported):
            _note(str(ent[2]))
            raise ent[2]
        return _hit(ent[2], _path)
    try:
        if not fns:
            raise Unsupported("an empty list of callables")
        if len(fns) > runtime.MAX_SPLIT:
            raise Unsupported("%d subsets: the split kernel builds in at most %d callables" % (len(fns), runtime.MAX_SPLIT))
        traced = []
        for m, fn in enumerate(fns):
            try:
                if not callable(fn):
                    raise Unsupported("not a callable")
                tr = trace_callback(fn, example)
                stats["traced"] += 1
                _too_large_unrolled(tr, runtime.MAX_SPLIT_NODES, "lists of callables under the split integrators")
                _check_against_autograd(tr, fn, example)
            except Unsupported as e:
                raise Unsupported("subset %d: %s" % (m, e)) from None
            traced.append(tr)
        out = CompiledSplit(traced, runtime.split_generated_source(traced, dtype, mass_kind), runtime.SKELETON_SPLIT, dtype, mass_kind)
        ret = _finish(out, _path)
    except Unsupported as e:
        stats["unsupported"] += 1
        _note(str(e))
        out = e
    if sig is not None:
        try:
            with _lock:
                _by_fn.setdefault(fns[0], {})[cfg] = (sig, objs, out, refs)
        except TypeError:
            pass
    if isinstance(out, Unsupported):
        raise out
    return ret


def _check_against_autograd(traced, fn, example, points=4, evaluate=None):
    """A fresh trace is believed only after its VALUE AND GRADIENT (the graph's own reverse mode, evaluated in numpy) reproduce the callable
    under torch.autograd at a few points around the example.  The trace records operations, not autograd semantics: a `torch.no_grad()`
    block, a custom `autograd.Function` backward or a gradient hook inside the callable would compile to the derivative of what is
    COMPUTED, not to what autograd returns - such callables are refused here (the run-time check of sample() compares values only).
    `evaluate(points[k, D]) -> [k, 1 + D]` replaces the graph's own value + gradient: the rolled program's interpreter (roll.py)."""
    import numpy as np
    g = torch.Generator(device="cpu").manual_seed(0x5EED)
    base = example.detach().double().cpu()
    pts = torch.cat([base[None], base[None] + 0.05 * (1.0 + base.abs())[None] * torch.randn(points - 1, base.numel(), generator=g, dtype=torch.float64)])
    if evaluate is None:
        grads = traced.grad()
        mine = traced.graph.evaluate([traced.value] + grads, pts.numpy(), np.float64)
    else:
        mine = evaluate(pts.numpy())
    tol = 2e-3 if example.dtype == torch.float32 else 1e-7
    for k in range(pts.shape[0]):
        x = pts[k].to(device=example.device, dtype=example.dtype).requires_grad_(True)
        try:
            with torch.enable_grad():
                v = fn(x)
                v = v.sum() if v.dim() else v
                gr, = torch.autograd.grad(v, x, allow_unused=True)
        except Exception as e:
            raise Unsupported("autograd of the callable failed at a check point (%s)" % str(e).split("\n")[0][:100]) from None
        ref = np.concatenate([[float(v)], (torch.zeros_like(x) if gr is None else gr).detach().double().cpu().numpy()])
        if not np.all(np.isfinite(ref)) or not np.all(np.isfinite(mine[k])):
            continue
        if np.abs(mine[k] - ref).max() > tol * (1.0 + np.abs(ref).max()):
            raise Unsupported("the traced graph's value / gradient disagree with torch.autograd at a check point (max difference %.3g): "
                              "a no_grad block, a custom backward or a hook inside the callable?" % np.abs(mine[k] - ref).max())


def torch_logp(fn, theta):
    """log p of every row of theta [k, D] by the callable itself (torch, no graphs): the reference the compiled code is checked against."""
    def f(w):
        r = fn(w)
        r = r[0] if isinstance(r, tuple) else r
        return r.sum() if torch.is_tensor(r) and r.dim() else r
    with torch.no_grad():
        try:
            return torch.func.vmap(f)(theta)
        except Exception:
            return torch.stack([torch.as_tensor(f(t)) for t in theta])
