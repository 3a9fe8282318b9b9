"""CPU: the callback compiler for LISTS of callables (Integrator.SPLITTING / SPLITTING_RAND / SPLITTING_KMID) up to and including
the gfx950 code object - no GPU needed.

* every subset's lowered value and gradient against the callable itself under torch.autograd;
* the generated include + csrc/jit/split_callback.hip.in through hipRTC: float32 / float64, mass kinds 0 / 1 / 2; the code object
  exports hta_cb_split_kernel and the info block, nothing goes to scratch, and every generated body is in it ONCE (the text grows
  by one body per added subset, not by one per kick);
* the refusals (mixed D, more than 16 subsets, a subset with data-dependent control flow - named -, too many operations);
* the single-callable skeleton after its helpers moved into the shared header: same exported symbols.
"""
import re
import subprocess

import numpy as np
import pytest
import torch

from hamiltorch_amd import jit
from hamiltorch_amd.jit import emit, runtime
from hamiltorch_amd.jit.ir import Unsupported
from hamiltorch_amd.jit.trace import trace_callback

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
f64 = torch.float64
D = 6


def logistic_list(M, rows=8, dtype=f64, d=D):
    """Bayesian logistic regression split into M subsets of `rows` rows: plain closures over tensors (no `_hta_spec`)."""
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
    regs = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", notes)}
    text = int(re.search(r"\.text\s+PROGBITS\s+\S+\s+\S+\s+([0-9a-f]+)", sec).group(1), 16)
    return sym, regs, text


def test_every_subset_of_the_list_lowers_to_the_callable():
    fns = logistic_list(3)
    trs = traces(fns)
    src = emit.split_value_grad_source(trs, "f64", 0)
    assert "#define HTA_CB_M 3" in src and "#define HTA_CB_D %d" % D in src
    for m in range(3):
        assert "void value_grad_%d(" % m in src and "void value_%d(" % m in src
    assert src.count("void value_grad_m(int m") == 1 and src.count("void value_m(int m") == 1
    live = [len(t.graph.reachable([t.value] + t.grad())) for t in trs]
    assert "#define HTA_CB_NODES %d" % sum(live) in src
    pts = 0.8 * torch.randn(20, D, dtype=f64, generator=torch.Generator().manual_seed(3))
    for f, t in zip(fns, trs):
        got = t.graph.evaluate([t.value] + t.grad(), pts.numpy(), np.float64)
        for k, x in enumerate(pts):
            x = x.clone().requires_grad_(True)
            v = f(x)
            g, = torch.autograd.grad(v, x)
            np.testing.assert_allclose(got[k, 0], float(v.detach()), rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(got[k, 1:], g.numpy(), rtol=1e-10, atol=1e-11)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mass", [0, 1, 2])
def test_the_list_compiles_for_gfx950(dtype, mass, tmp_path):
    src = runtime.split_generated_source(traces(logistic_list(3)), dtype, mass)
    key, blob = runtime.compile_source(src, runtime.SKELETON_SPLIT)
    sym, regs, _ = inspect(blob, tmp_path)
    assert "hta_cb_split_kernel" in sym and "hta_cb_info" in sym and "hta_cb_hmc_kernel" not in sym
    assert regs["vgpr_spill_count"] == 0 and regs["private_segment_fixed_size"] == 0, regs
    assert runtime.compile_source(src, runtime.SKELETON_SPLIT)[0] == key                       # cached by content


def test_each_generated_body_is_in_the_code_object_once(tmp_path):
    """One call site of the gradient dispatcher in the stage loop: the kernel's text grows by ONE body per added subset.  A step has 2 M
    kicks; bodies inlined at every kick would make the text grow like 2 M * M (M = 3 -> 6: four times; one body per subset: twice)."""
    text = {}
    for M in (3, 6, 12):
        _, blob = runtime.compile_source(runtime.split_generated_source(traces(logistic_list(M)), torch.float32, 0), runtime.SKELETON_SPLIT)
        _, regs, text[M] = inspect(blob, tmp_path)
        assert regs["private_segment_fixed_size"] == 0
    per_body = (text[6] - text[3]) / 3.0
    assert per_body > 0
    assert abs((text[12] - text[6]) / 6.0 - per_body) <= 0.25 * per_body, text           # linear in M
    assert text[3] <= 3 * per_body * 1.6, text                                            # M = 3: three bodies + the skeleton, not 6 x 3


def test_refusals_say_why_and_name_the_subset():
    fns = logistic_list(3)
    ex = torch.ones(D, dtype=f64)

    def branchy(w):
        return (w * w).sum() if w[0] > 0 else -(w * w).sum()

    with pytest.raises(Unsupported, match=r"subset 2: .*control flow"):
        jit.compile_split([fns[0], fns[1], branchy], ex, f64, 0)
    assert "subset 2" in jit.last_reason()
    with pytest.raises(Unsupported, match="at most 16"):
        jit.compile_split(logistic_list(17), ex, f64, 0)
    with pytest.raises(Unsupported, match="at most 16"):
        runtime.split_generated_source(traces(logistic_list(17)), f64, 0)
    mixed = traces(fns[:2]) + [trace_callback(lambda w: -(w * w).sum(), torch.ones(D + 1, dtype=f64))]
    with pytest.raises(Unsupported, match="do not share one parameter vector"):
        runtime.split_generated_source(mixed, f64, 0)
    big = traces(logistic_list(4, rows=160))
    assert sum(len(t.graph.reachable([t.value] + t.grad())) for t in big) > runtime.MAX_SPLIT_NODES
    with pytest.raises(Unsupported, match="scalar operations in all"):
        runtime.split_generated_source(big, f64, 0)
    with pytest.raises(Unsupported, match="registers"):
        runtime.split_generated_source([trace_callback(lambda w: -(w * w).sum(), torch.ones(200))] * 2, torch.float32, 0)


def test_compiled_lists_are_reused_by_the_tuple_of_closure_signatures():
    scale = torch.tensor(2.0, dtype=f64)
    fns = logistic_list(2) + [lambda w: -scale * (w ** 4).sum()]
    ex = torch.ones(D, dtype=f64)
    t0, h0 = jit.stats["traced"], jit.stats["trace_hits"]
    a = jit.compile_split(fns, ex, f64, 0)
    assert a.M == 3 and jit.stats["traced"] == t0 + 3
    assert jit.compile_split(fns, ex, f64, 0) is a and jit.stats["trace_hits"] == h0 + 1
    scale.mul_(2.0)                                              # ONE member's closure moved: the list is traced again
    c = jit.compile_split(fns, ex, f64, 0)
    assert c is not a and c.key != a.key and jit.stats["traced"] == t0 + 6
    assert jit.compile_split(fns[::-1], ex, f64, 0) is not c     # another order is another kernel
    assert jit.compile_split(fns, ex, f64, 1) is not c           # and so is another mass kind
    assert jit.compile_split(fns, ex, f64, 0, fresh=True) is not c


def test_single_callable_skeleton_exports_the_same_symbols(tmp_path):
    """apply_inv_mass / kinetic / drift / draw_momentum now come from csrc/jit/cb_hmc_shared.hpp: the plain-HMC code object still has
    both kernels and the info block, and spills nothing."""
    assert ("cb_hmc_shared.hpp", "jit/cb_hmc_shared.hpp") in runtime._HEADERS
    tr = trace_callback(logistic_list(1)[0], torch.ones(D, dtype=f64))
    for dtype, mass in ((torch.float32, 0), (torch.float64, 2)):
        _, blob = runtime.compile_source(runtime.hmc_generated_source(tr, dtype, mass), runtime.SKELETON_HMC)
        sym, regs, _ = inspect(blob, tmp_path)
        assert "hta_cb_hmc_kernel" in sym and "hta_cb_predraw_kernel" in sym and "hta_cb_info" in sym and "hta_cb_split_kernel" not in sym
        assert regs["vgpr_spill_count"] == 0 and regs["private_segment_fixed_size"] == 0, regs
