"""Compile traced callbacks with hipRTC (through the C ABI) and keep the results.

``compile_source`` turns generated text + the hand-written skeleton under ``csrc/jit/`` into a gfx950 code object
(``hta_jit_compile``; host work, needs no GPU - the CPU tests compile every example this way); ``Module`` loads one on a
device (``hta_jit_load``).  Code objects are cached by the hash of everything that went into them, modules by (hash, device).
"""
from __future__ import annotations

import ctypes
import hashlib
import os
import threading

import torch

from .. import _abi
from . import emit
from .ir import Unsupported

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
_HEADERS = (("cb_math.hpp", "jit/cb_math.hpp"), ("philox.hpp", "philox.hpp"), ("mh_rules.hpp", "mh_rules.hpp"),
            ("jit_args.h", "jit/jit_args.h"), ("cb_hmc_shared.hpp", "jit/cb_hmc_shared.hpp"),
            ("cb_hmc_bodies.inc", "jit/cb_hmc_bodies.inc"),
            ("rmhmc_metric_softabs.inc", "jit/rmhmc_metric_softabs.inc"), ("rmhmc_metric_hessian.inc", "jit/rmhmc_metric_hessian.inc"))
SKELETON_HMC = "jit/hmc_callback.hip.in"
SKELETON_SPLIT = "jit/split_callback.hip.in"
SKELETON_PATH = "jit/path_callback.hip.in"
SKELETON_ROLLED = "jit/rolled_callback.hip.in"
SKELETON_DERIVS = "jit/derivs_callback.hip.in"
SKELETON_RMHMC = "jit/rmhmc_callback.hip.in"      # both metrics: HTA_CB_METRIC of the generated include picks rmhmc_metric_*.inc
SKELETON_RMHMC_IMPLICIT = "jit/rmhmc_implicit_callback.hip.in"      # the implicit integrator over the same include and metric files
# (SLP vectorisation ON: the straight-line callback code packs into v_pk_mul / v_pk_fma pairs - 67 -> 59 instructions per
#  leapfrog step of the notebook funnel, tools/jit_isa.py; -ffp-contract=fast fuses across the generated statements)
OPTIONS = ("--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast")

_lock = threading.Lock()
_text = {}
_code = {}          # sha1 -> bytes (gfx950 code object); the 64 most recently used
MAX_CODE = 64
_modules = {}       # (sha1, device index) -> Module
stats = {"compiled": 0, "code_hits": 0, "loaded": 0, "compile_seconds": 0.0}


class CompileError(RuntimeError):
    """hipRTC rejected generated code (a bug of the emitter, or a device function hipRTC lacks); `log` has its messages."""

    def __init__(self, msg, log):
        super().__init__(msg)
        self.log = log


def _read(rel):
    t = _text.get(rel)
    if t is None:
        with open(os.path.join(_CSRC, rel)) as f:
            t = _text[rel] = f.read()
    return t


def compile_source(generated, skeleton):
    """(sha1, code-object bytes) of `skeleton` (a file under csrc/) compiled with `generated` as "hta_cb_generated.inc"."""
    import time
    main = _read(skeleton)
    headers = [(n, _read(rel)) for n, rel in _HEADERS] + [("hta_cb_generated.inc", generated)]
    h = hashlib.sha1()
    for part in (main,) + tuple(t for _, t in headers) + OPTIONS:
        h.update(part.encode()); h.update(b"\0")
    key = h.hexdigest()
    with _lock:
        hit = _code.pop(key, None)
        if hit is not None:
            _code[key] = hit            # most recently used last
    if hit is not None:
        stats["code_hits"] += 1
        return key, hit
    lib = _abi.load()
    n = len(headers)
    names = (ctypes.c_char_p * n)(*[a.encode() for a, _ in headers])
    srcs = (ctypes.c_char_p * n)(*[b.encode() for _, b in headers])
    opts = (ctypes.c_char_p * len(OPTIONS))(*[o.encode() for o in OPTIONS])
    code, size = ctypes.c_void_p(), ctypes.c_int64(0)
    t0 = time.perf_counter()
    rc = lib.hta_jit_compile(main.encode(), os.path.basename(skeleton).encode(), n, names, srcs, len(OPTIONS), opts,
                             ctypes.byref(code), ctypes.byref(size))
    stats["compile_seconds"] += time.perf_counter() - t0
    if rc != 0:
        log = lib.hta_jit_last_log().decode("utf-8", "replace")
        msg = "hamiltorch_amd: hta_jit_compile failed (%d): %s" % (rc, _abi.last_error())
        if rc == -3:
            raise Unsupported(msg)
        raise CompileError(msg + "\n" + log[-4000:], log)
    try:
        blob = ctypes.string_at(code.value, size.value)
    finally:
        lib.hta_jit_free(code)
    with _lock:
        while len(_code) >= MAX_CODE:
            _code.pop(next(iter(_code)))
        _code[key] = blob
    stats["compiled"] += 1
    return key, blob


class Module:
    """A code object loaded on one device (hta_jit_load); unloaded with the object."""

    def __init__(self, blob, device):
        self.device = torch.device(device)
        self._blob = blob                       # (hipModuleLoadData reads it during the call only; kept for reloads / debugging)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _abi._check(_abi.load().hta_jit_load(blob, len(blob), ctypes.byref(h)), "hta_jit_load")
        self.handle = h
        info = (ctypes.c_int * 8)()
        _abi._check(_abi.load().hta_jit_module_info(h, info), "hta_jit_module_info")
        self.info = list(info)
        stats["loaded"] += 1

    def __del__(self):
        try:
            if self.handle:
                _abi.load().hta_jit_unload(self.handle)
                self.handle = None
        except Exception:       # interpreter shutdown
            pass


def module_for(key, blob, device):
    device = torch.device(device)
    k = (key, device.index if device.index is not None else torch.cuda.current_device())
    with _lock:
        m = _modules.get(k)
    if m is None:
        m = Module(blob, device)
        with _lock:
            if len(_modules) >= 64:
                _modules.pop(next(iter(_modules)))
            _modules[k] = m
    return m


def dtype_name(dtype):
    if dtype == torch.float32:
        return "f32"
    if dtype == torch.float64:
        return "f64"
    raise Unsupported("compiled callbacks compute in float32 or float64, got %s" % dtype)


# ---- HMC ------------------------------------------------------------------------------------------------------------
MAX_HMC_DIM = 64                # value + gradient + state in one lane's registers
MAX_HMC_NODES = 6000            # live scalar operations of value + gradient (straight-line code in every lane)


def hmc_generated_source(traced, dtype, mass_kind):
    D = traced.D
    if D > MAX_HMC_DIM:
        raise Unsupported("D = %d: the chain-per-lane kernel holds theta, p and the gradient in registers (D <= %d)" % (D, MAX_HMC_DIM))
    grads = traced.grad()
    live = len(traced.graph.reachable([traced.value] + grads))
    if live > MAX_HMC_NODES:
        raise Unsupported("value + gradient are %d scalar operations (limit %d)" % (live, MAX_HMC_NODES))
    return emit.value_grad_source(traced.graph, traced.value, grads, dtype_name(dtype), mass_kind)


def hmc_predraw_bytes(C, D, n_traj, itemsize):
    return int(_abi.load().hta_jit_hmc_predraw_bytes(int(C), int(D), int(n_traj), int(itemsize)))


def hmc_workspace_bytes(C, D, itemsize):
    return int(_abi.load().hta_jit_hmc_workspace_bytes(int(C), int(D), int(itemsize)))


def _fill_common(a, cur, init, inv_mass, mass_factor, L, eps, n_traj, traj_offset, burn, seed, chain_offset, samples, reject_count,
                 H_old, H_new, accept, resume, pre=None):
    """The fields HtaCbHmcArgs and HtaCbRolledArgs share (csrc/jit/jit_args.h: HTA_CB_HMC_FIELDS); returns (C, D)."""
    _abi.require_device(cur, "params")
    C, D = cur.shape
    a.cur, a.init = cur.data_ptr(), _abi._p(init, cur).value
    a.inv_mass = None if inv_mass is None else _abi._p(inv_mass, cur).value
    a.mass_factor = None if mass_factor is None else _abi._p(mass_factor, cur).value
    a.samples = None if samples is None else _abi._p(samples, cur).value
    a.reject_count = reject_count.data_ptr()
    a.H_old = None if H_old is None else _abi._p(H_old, cur).value
    a.H_new = None if H_new is None else _abi._p(H_new, cur).value
    a.accept = None if accept is None else accept.data_ptr()
    a.C, a.eps, a.seed, a.chain_offset = C, float(eps), int(seed) & 0xFFFFFFFFFFFFFFFF, int(chain_offset)
    a.L, a.n_traj, a.traj_offset, a.burn = int(L), int(n_traj), int(traj_offset), int(burn)
    a.resume = 1 if resume else 0
    if pre is not None:
        a.pre, a.pre_bytes = pre.data_ptr(), pre.numel() * pre.element_size()
    return C, D


def hmc_sample(module, cur, init, mass_kind, inv_mass, mass_factor, L, eps, n_traj, traj_offset, burn, seed, chain_offset,
               samples, reject_count, workspace, H_old=None, H_new=None, accept=None, resume=False, pre=None):
    """hta_jit_hmc_sample: trajectories [traj_offset, traj_offset + n_traj) on the compiled callback, one launch."""
    a = _abi.HtaCbHmcArgs()
    C, D = _fill_common(a, cur, init, inv_mass, mass_factor, L, eps, n_traj, traj_offset, burn, seed, chain_offset, samples, reject_count,
                        H_old, H_new, accept, resume, pre)
    with torch.cuda.device(cur.device):
        _abi._check(_abi.load().hta_jit_hmc_sample(module.handle, ctypes.byref(a), D, cur.element_size(), int(mass_kind),
                                                   workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                                   _abi._stream(cur)), "hta_jit_hmc_sample")


def hmc_final_logp(workspace, C, D, dtype):
    """log p at the state the last launch ended in ([C] view of the workspace's second block)."""
    item = torch.empty((), dtype=dtype).element_size()
    return workspace[C * D * item:C * D * item + C * item].view(dtype)


# ---- plain HMC on a callable rolled over its data rows (roll.py) -----------------------------------------------------------
ROLLED_WAVES = (1, 2, 4, 8, 16)  # W: waves of one workgroup of 64 chains (csrc/jit/rolled_callback.hip.in)
ROLLED_LDS = 64 << 10           # bytes of dynamic LDS of one workgroup at most (HTA_CB_ROLLED_LDS)
ROLLED_TABLE_DEFAULT = "direct"
ROLLED_MAX_WAVES_GRID = 2048    # waves of one launch that share the row loops (beyond: the chains fill the machine themselves)


# The rolled route is OPT-IN until its rate is measured against the torch-evaluated route on the workload of tools/jit_roll_rate.py
# (profiles/r09a_rolled.json holds no rates yet): a default must not be slower than what it replaces.  'auto' is what the default
# becomes once those numbers exist and favour it.
ROLL_DEFAULT = "0"


def roll_mode():
    """HAMILTORCH_AMD_JIT_ROLL: 'auto' (roll where the straight-line route refuses for size), '0' (never), 'force' (whenever a
    group exists: tests at small shapes); unset: ROLL_DEFAULT."""
    m = os.environ.get("HAMILTORCH_AMD_JIT_ROLL", ROLL_DEFAULT).strip().lower()
    return m if m in ("0", "force", "auto") else ROLL_DEFAULT


def rolled_table_mode():
    """HAMILTORCH_AMD_JIT_ROLL_TABLE: how the row loop reads a group's table - 'direct' (wave-uniform loads from global memory) or
    'lds' (a tile of rows per wave staged through LDS); csrc/jit/rolled_callback.hip.in.  The default is the faster of the two on the
    workload of tools/jit_roll_rate.py."""
    m = os.environ.get("HAMILTORCH_AMD_JIT_ROLL_TABLE", ROLLED_TABLE_DEFAULT).strip().lower()
    return m if m in ("direct", "lds") else ROLLED_TABLE_DEFAULT


def rolled_max_waves(D, itemsize, live=0):
    """The waves per workgroup the rolled kernel is BUILT for (its launch bound): every wave holds theta, p, the gradient, the
    pre-drawn record and the partial sums in registers next to the term's temporaries, and a workgroup of 16 / 8 / 4 waves leaves a
    lane 128 / 256 / 512 registers (4 waves: what the straight-line kernel has).  `live`: the live operations of the largest term
    with its gradient.  Logistic / Gaussian terms (20 - 60 operations) take 64 + 6 D registers in float32 and 110 + 10 D in float64
    (double-precision log and exp): no scratch within the first bounds below, tests/test_jit_roll_cpu.py.  A heavier term gets the
    wider register budget instead of more waves - a heuristic: beyond it the compiler spills, which is slower and not wrong."""
    if itemsize == 4:
        return 16 if (D <= 10 and live <= 80) else (8 if (D <= 30 and live <= 250) else 4)
    return 8 if (D <= 12 and live <= 120) else 4


def rolled_waves(C, D, U, max_rows, itemsize, live=0):
    """THE rule for W: the largest of ROLLED_WAVES for which the partial sums fit the LDS bound (W * 64 * (1 + D + U) * itemsize <=
    64 KB), every wave has at least 8 rows of the largest group (W <= rows / 8), the launch has at most 2048 waves
    (ceil(C / 64) * W) and the kernel's launch bound holds (rolled_max_waves)."""
    blocks = -(-int(C) // 64)
    best = 1
    for W in ROLLED_WAVES:
        if (W * 64 * (1 + D + U) * itemsize <= ROLLED_LDS and W * 8 <= max_rows and blocks * W <= ROLLED_MAX_WAVES_GRID
                and W <= rolled_max_waves(D, itemsize, live)):
            best = W
    return best


def rolled_program(traced):
    """roll.Rolled of a traced callable under the limits of the rolled kernel; raises Unsupported with the reason."""
    from . import roll
    if traced.D > MAX_HMC_DIM:
        raise Unsupported("D = %d: the chain-per-lane kernel holds theta, p and the gradient in registers (D <= %d)" % (traced.D, MAX_HMC_DIM))
    return roll.roll(traced.graph, traced.value, MAX_HMC_NODES)


def rolled_generated_source(rolled, dtype, mass_kind):
    """The generated include of csrc/jit/rolled_callback.hip.in for a roll.Rolled program."""
    item = torch.empty((), dtype=dtype).element_size()
    live = max(g.live for g in rolled.groups)
    return emit.rolled_value_grad_source(rolled, dtype_name(dtype), mass_kind, rolled_max_waves(rolled.D, item, live),
                                         rolled_table_mode() == "lds")


def rolled_sample(module, cur, init, U, tables, rows, waves, mass_kind, inv_mass, mass_factor, L, eps, n_traj, traj_offset, burn, seed,
                  chain_offset, samples, reject_count, workspace, H_old=None, H_new=None, accept=None, resume=False, pre=None):
    """hta_jit_rolled_sample: trajectories [traj_offset, traj_offset + n_traj) on the rolled callback, one launch; `tables` are the
    groups' device tables ([rows, slots] in the run's dtype), `waves` the waves per workgroup of 64 chains."""
    a = _abi.HtaCbRolledArgs()
    C, D = _fill_common(a, cur, init, inv_mass, mass_factor, L, eps, n_traj, traj_offset, burn, seed, chain_offset, samples, reject_count,
                        H_old, H_new, accept, resume, pre)
    for k, (t, r) in enumerate(zip(tables, rows)):
        a.table[k], a.rows[k] = _abi._p(t, cur).value, int(r)
    a.waves = int(waves)
    with torch.cuda.device(cur.device):
        _abi._check(_abi.load().hta_jit_rolled_sample(module.handle, ctypes.byref(a), D, int(U), len(tables), cur.element_size(),
                                                      int(mass_kind), workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                                      _abi._stream(cur)), "hta_jit_rolled_sample")


# ---- split HMC on a list of callables ---------------------------------------------------------------------------------
MAX_SPLIT = 16                  # subsets of one compiled list (HTA_CB_MAX_SPLIT: a subset order packs into 64 bits)
MAX_SPLIT_NODES = MAX_HMC_NODES  # SUM of the subsets' live value + gradient operations


def split_generated_source(traced_list, dtype, mass_kind):
    """The generated include of csrc/jit/split_callback.hip.in for a list of traced callables (one per data subset)."""
    M = len(traced_list)
    if M < 1:
        raise Unsupported("an empty list of callables")
    if M > MAX_SPLIT:
        raise Unsupported("%d subsets: the split kernel builds in at most %d callables" % (M, MAX_SPLIT))
    dims = [t.D for t in traced_list]
    if len(set(dims)) != 1:
        raise Unsupported("the subsets do not share one parameter vector (D = %s)" % ", ".join(str(d) for d in dims))
    D = dims[0]
    if D > MAX_HMC_DIM:
        raise Unsupported("D = %d: the chain-per-lane kernel holds theta, p and the gradient in registers (D <= %d)" % (D, MAX_HMC_DIM))
    live = [len(t.graph.reachable([t.value] + t.grad())) for t in traced_list]
    if sum(live) > MAX_SPLIT_NODES:
        raise Unsupported("value + gradient of the %d subsets are %d scalar operations in all (limit %d)" % (M, sum(live), MAX_SPLIT_NODES))
    return emit.split_value_grad_source(traced_list, dtype_name(dtype), mass_kind)


def split_workspace_bytes(C, D, itemsize):
    return int(_abi.load().hta_jit_split_workspace_bytes(int(C), int(D), int(itemsize)))


def split_sample(module, cur, init, M, split_kind, mass_kind, inv_mass, mass_factor, L, eps, n_traj, traj_offset, burn, seed,
                 chain_offset, samples, reject_count, workspace, H_old=None, H_new=None, accept=None, resume=False):
    """hta_jit_split_sample: trajectories [traj_offset, traj_offset + n_traj) of a split integrator on the compiled list, one launch."""
    a = _abi.HtaCbHmcArgs()
    C, D = _fill_common(a, cur, init, inv_mass, mass_factor, L, eps, n_traj, traj_offset, burn, seed, chain_offset, samples, reject_count,
                        H_old, H_new, accept, resume)
    a.split_kind = int(split_kind)
    with torch.cuda.device(cur.device):
        _abi._check(_abi.load().hta_jit_split_sample(module.handle, ctypes.byref(a), D, int(M), cur.element_size(), int(mass_kind),
                                                     int(split_kind), workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                                     _abi._stream(cur)), "hta_jit_split_sample")


def split_final_logp(workspace, C, dtype):
    """Sum of the subsets' log p at the state the last launch ended in ([C] view of the workspace)."""
    item = torch.empty((), dtype=dtype).element_size()
    return workspace[:C * item].view(dtype)


# ---- leapfrog paths (samplers.leapfrog on a batch of chains) -----------------------------------------------------------
def path_generated_source(traced_or_list, dtype, mass_kind):
    """The generated include of csrc/jit/path_callback.hip.in: that of the trajectory kernels, text for text - a traced callable
    gives hmc_generated_source (hta_cb_path_kernel), a list of them split_generated_source (hta_cb_split_path_kernel) - with
    their limits and refusals."""
    if isinstance(traced_or_list, (list, tuple)):
        return split_generated_source(list(traced_or_list), dtype, mass_kind)
    return hmc_generated_source(traced_or_list, dtype, mass_kind)


def path_leapfrog(module, theta0, p0, M, split_kind, mass_kind, inv_mass, steps, eps, seed, path_theta, path_p, lp_end=None):
    """hta_jit_path_leapfrog: every step of one leapfrog call from (theta0, p0) [C, D] into path_theta / path_p [steps, C, D] and
    log p at the end points into lp_end [C], one launch.  M = 0: a single callable; else a list of M under split_kind."""
    _abi.require_device(theta0, "params")
    C, D = theta0.shape
    a = _abi.HtaCbPathArgs()
    a.theta0, a.p0 = theta0.data_ptr(), _abi._p(p0, theta0).value
    a.inv_mass = None if inv_mass is None else _abi._p(inv_mass, theta0).value
    a.path_theta, a.path_p = _abi._p(path_theta, theta0).value, _abi._p(path_p, theta0).value
    a.lp_end = None if lp_end is None else _abi._p(lp_end, theta0).value
    a.C, a.eps, a.seed = C, float(eps), int(seed) & 0xFFFFFFFFFFFFFFFF
    a.steps, a.split_kind = int(steps), int(split_kind)
    with torch.cuda.device(theta0.device):
        _abi._check(_abi.load().hta_jit_path_leapfrog(module.handle, ctypes.byref(a), D, int(M), theta0.element_size(), int(mass_kind),
                                                      int(split_kind), _abi._stream(theta0)), "hta_jit_path_leapfrog")


# ---- derivatives for the Riemannian samplers ---------------------------------------------------------------------------
MAX_DERIV_DIM = 32
MAX_DERIV_NODES = 20000         # live scalar operations of each generated function


MAX_RMHMC_DIM = 16              # a chain's matrices in one lane's registers (csrc/jit/rmhmc_callback.hip.in)


def derivs_generated_source(traced, dtype, jitter=False, metric=None):
    """Value, gradient, Hessian (D reverse passes over the gradient's graph) and the third derivatives (one pass per Hessian
    entry of the lower triangle) of a traced callable, as the generated include of csrc/jit/derivs_callback.hip.in - and, with
    `metric` ("softabs" | "hessian"), of the RMHMC trajectory skeleton (SKELETON_RMHMC), which takes
    its metric from the include (none: soft-abs)."""
    D = traced.D
    if D > MAX_DERIV_DIM:
        raise Unsupported("D = %d: third derivatives are generated entry by entry (D <= %d)" % (D, MAX_DERIV_DIM))
    g = traced.graph
    grads = traced.grad()
    hess = [g.grad(gi) for gi in grads]
    if len(g.reachable([traced.value] + grads + [hess[i][j] for i in range(D) for j in range(i + 1)])) > MAX_DERIV_NODES:
        raise Unsupported("value + gradient + Hessian exceed %d scalar operations" % MAX_DERIV_NODES)
    # Two forms of the third derivatives behind third_contract.  Entry by entry (one reverse pass per Hessian entry), a likelihood of R
    # terms costs R operations for each of the D^2 (D + 1) / 2 derivatives; the contraction they are wanted for is ONE scalar,
    # s = <Hessian(theta), M>, whose gradient by reverse mode costs a few times the Hessian itself.  The Metric.HESSIAN kernel takes
    # the second form; everything that compiled before it existed keeps the first - and its text - and either is the other's
    # fall-back where one is refused for its size.
    forms = (_contracted_third, _entrywise_third) if metric == "hessian" else (_entrywise_third, _contracted_third)
    try:
        third = forms[0](g, hess)
    except Unsupported as e:
        try:
            third = forms[1](g, hess)
        except Unsupported as e2:
            raise Unsupported("%s; %s" % ((e, e2) if forms[0] is _entrywise_third else (e2, e))) from None
    return emit.derivs_source(g, traced.value, grads, hess, third, dtype_name(dtype), jitter, metric)


def _entrywise_third(g, hess):
    """{(i, j), j <= i: the D derivatives of Hessian entry i, j}."""
    D = g.n_inputs
    third = {}
    for i in range(D):
        for j in range(i + 1):
            third[(i, j)] = g.grad(hess[i][j])
            if len(g.nodes) > 40 * MAX_DERIV_NODES:
                raise Unsupported("the third derivatives exceed the graph size limit")
    if len(g.reachable([t for v in third.values() for t in v])) > MAX_DERIV_NODES:
        raise Unsupported("the third derivatives exceed %d scalar operations" % MAX_DERIV_NODES)
    return third


def contracted_third(g, hess):
    """c_k = d_k sum_{i >= j} H_ij(theta) m_ij with the m_ij held fixed, as D nodes of `g`: m_ij enters as the EXTRA input
    D + i (i + 1) / 2 + j of the graph (emit.derivs_source fills it with M_ii, or M_ij + M_ji for an off-diagonal pair)."""
    D = g.n_inputs
    s = g.const(0.0)
    for i in range(D):
        for j in range(i + 1):
            s = g.add(s, g.mul(hess[i][j], g._new(("in", D + i * (i + 1) // 2 + j))))
    return g.grad(s)


def _contracted_third(g, hess):
    third = contracted_third(g, hess)
    live = len(g.reachable(third))
    if live > MAX_DERIV_NODES:
        raise Unsupported("the gradient of the contraction <Hessian, M> exceeds %d scalar operations (%d)" % (MAX_DERIV_NODES, live))
    return third


def rmhmc_workspace_bytes(C, D, itemsize):
    return int(_abi.load().hta_jit_rmhmc_workspace_bytes(int(C), int(D), int(itemsize)))


def rmhmc_sample(module, cur, init, L, eps, alpha, jitter, omega, n_traj, traj_offset, burn, seed, chain_offset, samples,
                 reject_count, workspace):
    """hta_jit_rmhmc_sample: explicit RMHMC trajectories [traj_offset, traj_offset + n_traj) on the compiled callable, under the metric
    the module was built for (soft-abs, or Metric.HESSIAN: `alpha` is not read and may be None)."""
    _abi.require_device(cur, "params")
    C, D = cur.shape
    a = _abi.HtaCbRmhmcArgs()
    a.cur, a.init = cur.data_ptr(), _abi._p(init, cur).value
    a.samples = None if samples is None else _abi._p(samples, cur).value
    a.reject_count = reject_count.data_ptr()
    a.C, a.eps, a.alpha, a.omega = C, float(eps), 0.0 if alpha is None else float(alpha), float(omega)
    a.jitter = 0.0 if jitter is None else float(jitter)
    a.seed, a.chain_offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(chain_offset)
    a.L, a.n_traj, a.traj_offset, a.burn = int(L), int(n_traj), int(traj_offset), int(burn)
    with torch.cuda.device(cur.device):
        _abi._check(_abi.load().hta_jit_rmhmc_sample(module.handle, ctypes.byref(a), D, cur.element_size(), 0 if jitter is None else 1,
                                                     workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                                     _abi._stream(cur)), "hta_jit_rmhmc_sample")


def rmhmc_implicit_sample(module, cur, init, L, eps, alpha, jitter, thr, max_it, n_traj, traj_offset, burn, seed, chain_offset, samples,
                          reject_count, workspace, iters=None):
    """hta_jit_rmhmc_implicit_sample: implicit RMHMC trajectories [traj_offset, traj_offset + n_traj) on the compiled callable, under the
    metric the module was built for (SKELETON_RMHMC_IMPLICIT).  `iters` (int32 [C], tests): accumulates the fixed-point iterations every
    chain executed while active."""
    _abi.require_device(cur, "params")
    C, D = cur.shape
    a = _abi.HtaCbRmhmcImpArgs()
    a.cur, a.init = cur.data_ptr(), _abi._p(init, cur).value
    a.samples = None if samples is None else _abi._p(samples, cur).value
    a.reject_count = reject_count.data_ptr()
    a.iters = None if iters is None else iters.data_ptr()
    a.C, a.eps, a.alpha = C, float(eps), 0.0 if alpha is None else float(alpha)
    a.jitter = 0.0 if jitter is None else float(jitter)
    a.thr, a.max_it = float(thr), int(max_it)
    a.seed, a.chain_offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(chain_offset)
    a.L, a.n_traj, a.traj_offset, a.burn = int(L), int(n_traj), int(traj_offset), int(burn)
    with torch.cuda.device(cur.device):
        _abi._check(_abi.load().hta_jit_rmhmc_implicit_sample(module.handle, ctypes.byref(a), D, cur.element_size(), 0 if jitter is None else 1,
                                                              workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                                              _abi._stream(cur)), "hta_jit_rmhmc_implicit_sample")


def _deriv_call(module, a, which, like):
    C, D = like.shape
    with torch.cuda.device(like.device):
        _abi._check(_abi.load().hta_jit_derivs(module.handle, ctypes.byref(a), int(which), D, like.element_size(), _abi._stream(like)),
                    "hta_jit_derivs")


def derivs(module, theta, logp, grad, neg_hess):
    """One launch: logp[C], grad[C, D], neg_hess[C, D, D] of the compiled callable at theta[C, D]."""
    _abi.require_device(theta, "params")
    a = _abi.HtaCbDerivArgs()
    a.theta, a.C = _abi._p(theta).value, theta.shape[0]
    a.logp = None if logp is None else _abi._p(logp, theta).value
    a.grad = None if grad is None else _abi._p(grad, theta).value
    a.neg_hess = _abi._p(neg_hess, theta).value
    _deriv_call(module, a, 0, theta)


def contract(module, theta, M, out=None, upd=None, grad_in=None, coef=0.0):
    """One launch: c = d < Hess log p (theta), M >|_(M fixed) per chain, to `out` and / or as upd += coef (grad_in + c)."""
    _abi.require_device(theta, "params")
    a = _abi.HtaCbDerivArgs()
    a.theta, a.C, a.M = _abi._p(theta).value, theta.shape[0], _abi._p(M, theta).value
    a.contract = None if out is None else _abi._p(out, theta).value
    a.upd = None if upd is None else _abi._p(upd, theta).value
    a.grad_in = None if grad_in is None else _abi._p(grad_in, theta).value
    a.coef = float(coef)
    _deriv_call(module, a, 1, theta)
