"""CPU: the callback compiler's leapfrog-PATH kernels (samplers.leapfrog on a (C, D) batch of chains) up to and including the gfx950
code object - no GPU needed.

* csrc/jit/path_callback.hip.in through hipRTC around the generated include of a single callable (hta_cb_path_kernel) and of a list
  (hta_cb_split_path_kernel): float32 / float64, mass kinds 0 / 1 / 2; the right kernel and the info block are exported, the other
  path kernel and the trajectory kernels are not, nothing spills and nothing goes to scratch;
* the trajectory kernels' code objects hold no path kernel, and the list's text still grows by ONE body per added subset;
* compile_path shares the trace cache of compile_hmc / compile_split, and refuses what they refuse, for their reasons;
* hta_jit_path_leapfrog turns bad arguments down before it looks at a device.
"""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

from hamiltorch_amd import _abi, jit
from hamiltorch_amd.jit import runtime
from hamiltorch_amd.jit.ir import Unsupported
from hamiltorch_amd.jit.trace import trace_callback

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
f64 = torch.float64
D = 6


def logistic_list(M, rows=8, dtype=f64, d=D):
    """Bayesian logistic regression split into M subsets of `rows` rows: plain closures over tensors."""
    rng = np.random.default_rng(0)
    X = rng.standard_normal((M * rows, d - 1))
    y = (rng.uniform(size=M * rows) > 0.5).astype(np.float64)
    fns = []
    for m in range(M):
        A = torch.tensor(X[m * rows:(m + 1) * rows], dtype=dtype)
        yy = torch.tensor(y[m * rows:(m + 1) * rows], dtype=dtype)

        def f(w, A=A, yy=yy):
            z = A @ w[:-1] + w[-1]
            return (yy * z - torch.nn.functional.softplus(z)).sum() - (0.5 / M) * (w * w).sum()
        fns.append(f)
    return fns


def traces(fns, d=D):
    return [trace_callback(f, torch.ones(d, dtype=f64)) for f in fns]


def inspect(blob, tmp_path):
    p = tmp_path / "cb.co"
    p.write_bytes(blob)
    sym = subprocess.run([READELF, "-s", str(p)], capture_output=True, text=True).stdout
    sec = subprocess.run([READELF, "-S", str(p)], capture_output=True, text=True).stdout
    notes = subprocess.run([READELF, "--notes", str(p)], capture_output=True, text=True).stdout
    # (a path code object holds ONE kernel - asserted through `names` - so these are that kernel's notes.  The bar is the sibling
    #  skeletons': no vector register spilled, no scratch.  Scalar registers parked in lanes of a vector register - float64 builds keep
    #  their constants in scalar pairs - cost no memory traffic; the trajectory kernels have more of them.)
    regs = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", notes)}
    text = int(re.search(r"\.text\s+PROGBITS\s+\S+\s+\S+\s+([0-9a-f]+)", sec).group(1), 16)
    names = set(re.findall(r"\b(hta_cb_\w+?)(?:\.kd)?\b", sym))
    return names, regs, text


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mass", [0, 1, 2])
def test_the_single_callable_path_kernel_compiles_for_gfx950(dtype, mass, tmp_path):
    tr = traces(logistic_list(1))[0]
    src = runtime.path_generated_source(tr, dtype, mass)
    assert src == runtime.hmc_generated_source(tr, dtype, mass)                 # the trajectory kernel's generated text, as it is
    key, blob = runtime.compile_source(src, runtime.SKELETON_PATH)
    names, regs, _ = inspect(blob, tmp_path)
    assert names == {"hta_cb_path_kernel", "hta_cb_info"}, names                # no split path kernel, no trajectory kernel
    assert regs["vgpr_spill_count"] == 0 and regs["private_segment_fixed_size"] == 0, regs
    assert runtime.compile_source(src, runtime.SKELETON_PATH)[0] == key         # cached by content
    assert runtime.compile_source(src, runtime.SKELETON_HMC)[0] != key


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mass", [0, 1, 2])
def test_the_list_path_kernel_compiles_for_gfx950(dtype, mass, tmp_path):
    trs = traces(logistic_list(3))
    src = runtime.path_generated_source(trs, dtype, mass)
    assert src == runtime.split_generated_source(trs, dtype, mass) and "#define HTA_CB_M 3" in src
    key, blob = runtime.compile_source(src, runtime.SKELETON_PATH)
    names, regs, _ = inspect(blob, tmp_path)
    assert names == {"hta_cb_split_path_kernel", "hta_cb_info"}, names
    assert regs["vgpr_spill_count"] == 0 and regs["private_segment_fixed_size"] == 0, regs
    assert runtime.compile_source(src, runtime.SKELETON_PATH)[0] == key


def test_the_trajectory_kernels_code_objects_hold_no_path_kernel(tmp_path):
    trs = traces(logistic_list(3))
    _, blob = runtime.compile_source(runtime.hmc_generated_source(trs[0], torch.float32, 0), runtime.SKELETON_HMC)
    names, _, _ = inspect(blob, tmp_path)
    assert names == {"hta_cb_hmc_kernel", "hta_cb_predraw_kernel", "hta_cb_info"}, names
    _, blob = runtime.compile_source(runtime.split_generated_source(trs, torch.float32, 0), runtime.SKELETON_SPLIT)
    names, _, _ = inspect(blob, tmp_path)
    assert names == {"hta_cb_split_kernel", "hta_cb_info"}, names


def test_each_generated_body_is_in_the_path_code_object_once(tmp_path):
    """One call site of the gradient dispatcher in the stage loop, as in the trajectory kernel: the text grows by ONE body per added
    subset.  Bodies inlined at every kick would make it grow like 2 M * M (M = 3 -> 6: four times; one body per subset: twice)."""
    text = {}
    for M in (3, 6, 12):
        _, blob = runtime.compile_source(runtime.path_generated_source(traces(logistic_list(M)), torch.float32, 0), runtime.SKELETON_PATH)
        _, regs, text[M] = inspect(blob, tmp_path)
        assert regs["private_segment_fixed_size"] == 0
    per_body = (text[6] - text[3]) / 3.0
    assert per_body > 0
    assert abs((text[12] - text[6]) / 6.0 - per_body) <= 0.25 * per_body, text           # linear in M
    assert text[3] <= 3 * per_body * 1.6, text                                            # M = 3: three bodies + the skeleton, not 6 x 3


def test_compile_path_shares_the_trace_cache_of_the_trajectory_kernels():
    ex = torch.ones(D, dtype=f64)
    fn = logistic_list(1)[0]
    t0, h0 = jit.stats["traced"], jit.stats["trace_hits"]
    a = jit.compile_hmc(fn, ex, f64, 0)
    assert jit.stats["traced"] == t0 + 1
    pa = jit.compile_path(fn, ex, f64, 0)
    assert isinstance(pa, jit.CompiledPath) and pa.M == 0 and pa.traced is a.traced and pa.key != a.key
    assert jit.stats["traced"] == t0 + 1 and jit.stats["trace_hits"] == h0 + 1
    assert jit.compile_path(fn, ex, f64, 0) is pa and jit.stats["traced"] == t0 + 1
    assert jit.compile_path(fn, ex, f64, 0, fresh=True) is not pa and jit.stats["traced"] == t0 + 2
    # the other way round: a callable first seen by leapfrog() is not traced again by sample()
    fns = logistic_list(3)
    t1, h1 = jit.stats["traced"], jit.stats["trace_hits"]
    pl = jit.compile_path(fns, ex, f64, 1)
    assert pl.M == 3 and pl.mass_kind == 1 and jit.stats["traced"] == t1 + 3
    s = jit.compile_split(fns, ex, f64, 1)
    assert jit.stats["traced"] == t1 + 3 and jit.stats["trace_hits"] == h1 + 1 and s.traced is pl.traced and s.key != pl.key
    assert jit.compile_path(fns, ex, f64, 1) is pl


def test_compile_path_refuses_what_the_trajectory_kernels_refuse():
    ex = torch.ones(D, dtype=f64)

    def branchy(w):
        return (w * w).sum() if w[0] > 0 else -(w * w).sum()

    with pytest.raises(Unsupported, match="control flow"):
        jit.compile_path(branchy, ex, f64, 0)
    assert "control flow" in jit.last_reason()
    with pytest.raises(Unsupported, match=r"subset 2: .*control flow"):
        jit.compile_path(logistic_list(2) + [branchy], ex, f64, 0)
    with pytest.raises(Unsupported, match=r"D = 65: .*registers \(D <= 64\)"):
        jit.compile_path(lambda w: -(w * w).sum(), torch.ones(65, dtype=f64), f64, 0)
    with pytest.raises(Unsupported, match=r"D = 65: .*registers \(D <= 64\)"):
        jit.compile_path([lambda w: -(w * w).sum(), lambda w: -(w ** 4).sum()], torch.ones(65, dtype=f64), f64, 0)
    with pytest.raises(Unsupported, match="at most 16"):
        jit.compile_path(logistic_list(17), ex, f64, 0)
    with pytest.raises(Unsupported, match="at most 16"):
        runtime.path_generated_source(traces(logistic_list(17)), f64, 0)
    with pytest.raises(Unsupported, match="registers"):
        runtime.path_generated_source(trace_callback(lambda w: -(w * w).sum(), torch.ones(65)), torch.float32, 0)


def test_the_entry_point_refuses_bad_arguments_without_a_device():
    lib = _abi.load()
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.addressof(buf)

    def call(module=None, M=0, D_=6, itemsize=8, mass=0, split_kind=0, **kw):
        a = _abi.HtaCbPathArgs()
        a.theta0 = a.p0 = a.path_theta = a.path_p = ptr
        a.C, a.eps, a.steps = 1, 0.1, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.hta_jit_path_leapfrog(module, ctypes.byref(a), D_, M, itemsize, mass, split_kind, None)

    assert ctypes.sizeof(_abi.HtaCbPathArgs) == 6 * 8 + 3 * 8 + 2 * 4          # pointers, 8-byte scalars, 4-byte scalars: no padding
    assert call() == -1 and "module is NULL" in _abi.last_error()
    assert lib.hta_jit_path_leapfrog(None, None, 6, 0, 8, 0, 0, None) == -1
    for bad in (dict(C=0), dict(steps=-1), dict(theta0=None), dict(p0=None), dict(D_=0), dict(itemsize=2), dict(path_theta=None),
                dict(path_p=None), dict(mass=3), dict(mass=1), dict(M=17), dict(M=-1), dict(split_kind=1), dict(M=3, split_kind=3),
                dict(M=1, split_kind=0), dict(M=1, split_kind=2)):
        assert call(**bad) == -1, bad
        assert "module is NULL" not in _abi.last_error(), bad                   # turned down for its own reason, before the module
    assert call(steps=0, path_theta=None, path_p=None) == 0                     # an empty path: nothing to launch
    assert call(steps=0, C=0) == -1
