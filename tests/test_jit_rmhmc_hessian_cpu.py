"""CPU half of the compiled Metric.HESSIAN trajectory kernel (csrc/jit/rmhmc_callback.hip.in with rmhmc_metric_hessian.inc): the
generated include and the skeleton build for gfx950 through hipRTC (no GPU needed), with no more scratch than the soft-abs kernel of the
same callable; the metric is part of the cache key and an include that names an unknown one does not compile; the third-derivative
contraction in its reverse-mode form equals the oracle's; and the oracle itself decides the cases of
tests/test_gpu_jit_rmhmc_hessian.py in float32 as in float64, far inside the float32 band.
"""
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import hmc_oracle as O
from hamiltorch_amd import jit
from hamiltorch_amd.jit import runtime
from hamiltorch_amd.jit.trace import trace_callback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
NP = {torch.float32: np.float32, torch.float64: np.float64}
N, L, EPS, OMEGA, SEED, OFF = 6, 3, 0.4, 10.0, 99, 7
CASES = [(70, 1, None, 0), (70, 2, 1e-3, 0), (70, 5, None, 2), (70, 8, 1e-2, -1), (70, 11, 1e-3, 0), (70, 16, 1e-2, 2), (1, 5, 1e-3, 0)]
HL2P = 0.9189385332046727


def target(D):
    """The log-cosh target of the GPU tests: default_rng(2) draws Q first, then A."""
    rng = np.random.default_rng(2)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    P = (Q * np.linspace(0.5, 2.0, D)) @ Q.T
    P = 0.5 * (P + P.T)
    return P, 0.6 * rng.standard_normal((D + 2, D))


def logcosh_logp(P, A):
    def f(w):
        Pt = torch.as_tensor(P, dtype=w.dtype, device=w.device); At = torch.as_tensor(A, dtype=w.dtype, device=w.device)
        return -0.5 * torch.dot(w, torch.mv(Pt, w)) - torch.log(torch.cosh(torch.mv(At, w))).sum()
    return f


def funnel(w):
    v, x = w[0], w[1:]
    return (-v * v / 18.0 - 1.0986122886681098 - HL2P) + (-0.5 * torch.exp(v) * (x * x).sum() + 0.5 * x.numel() * v - x.numel() * HL2P)


def _symbols(blob, tmp_path):
    p = tmp_path / "cb.co"
    p.write_bytes(blob)
    sym = subprocess.run([READELF, "-s", str(p)], capture_output=True, text=True).stdout
    notes = subprocess.run([READELF, "--notes", str(p)], capture_output=True, text=True).stdout
    regs = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", notes)}
    return sym, regs


def _header_constant(name):
    text = open(os.path.join(ROOT, "hamiltorch_amd", "csrc", "jit", "jit_args.h")).read()
    return int(re.search(r"#define %s (\w+)" % name, text).group(1), 0)


def built(D, dtype, jitter, metric, tmp_path):
    tr = trace_callback(logcosh_logp(*target(D)), torch.ones(D, dtype=torch.float64))
    src = runtime.derivs_generated_source(tr, dtype, jitter, metric)
    key, blob = runtime.compile_source(src, runtime.SKELETON_RMHMC)
    sym, regs = _symbols(blob, tmp_path)
    return src, blob, sym, regs


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("D", [1, 8, 16])
def test_symbols_and_resources(D, dtype, tmp_path):
    """The log-cosh target at D = 1, 8 and 16 (the register limit), jitter off and on: a gfx950 code object with
    hta_cb_rmhmc_hess_kernel and an info block of the new kernel set, and neither more spilled registers nor more scratch than the
    soft-abs kernel (csrc/jit/rmhmc_callback.hip.in) built around the same callable, D and dtype - the yardstick is the existing kernel.
    The counts are kept in profiles/r12a_rmhmc_hessian.json (tools/jit_rmhmc_hessian_rate.py resources)."""
    HTA_CB_MAGIC, HTA_CB_SET_RMHMC_HESS = _header_constant("HTA_CB_MAGIC"), _header_constant("HTA_CB_SET_RMHMC_HESS")
    _, _, sym0, yard = built(D, dtype, True, "softabs", tmp_path)
    assert "hta_cb_rmhmc_kernel" in sym0 and "hta_cb_rmhmc_hess_kernel" not in sym0
    item = 4 if dtype == torch.float32 else 8
    for jitter in (False, True):
        src, blob, sym, regs = built(D, dtype, jitter, "hessian", tmp_path)
        assert "#define HTA_CB_METRIC HTA_CB_METRIC_HESSIAN" in src and "#define HTA_CB_JITTER %d" % jitter in src
        assert "hta_cb_rmhmc_hess_kernel" in sym and "hta_cb_info" in sym
        assert struct.pack("<5i", HTA_CB_MAGIC, D, item, int(jitter), HTA_CB_SET_RMHMC_HESS) in blob       # hta_cb_info[0 .. 4]
        print("D=%d %s jitter=%d: hessian %s; soft-abs %s" % (D, runtime.dtype_name(dtype), jitter, regs, yard))
        assert regs["vgpr_spill_count"] <= yard["vgpr_spill_count"], (regs, yard)
        assert regs["private_segment_fixed_size"] <= yard["private_segment_fixed_size"], (regs, yard)


def test_the_metric_is_part_of_the_cache_key():
    """compile_rmhmc under the two metrics: two cache entries and two code objects of the one skeleton for one callable, each handed
    out again without a new trace; the soft-abs include is the parent's text plus the metric define."""
    P, A = target(3)
    fn, ex = logcosh_logp(P, A), torch.ones(3, dtype=torch.float32)
    traced = jit.stats["traced"]
    soft = jit.compile_rmhmc(fn, ex, torch.float32, True)
    hess = jit.compile_rmhmc(fn, ex, torch.float32, True, metric="hessian")
    assert soft is not hess and soft.key != hess.key
    assert soft.skeleton == hess.skeleton == runtime.SKELETON_RMHMC and soft.blob != hess.blob
    assert (soft.mass_kind, hess.mass_kind) == ("rmhmc-jitter", "rmhmc-hess-jitter")
    assert {cfg[2] for cfg in jit._by_fn[fn]} == {"rmhmc-jitter", "rmhmc-hess-jitter"}
    assert jit.compile_rmhmc(fn, ex, torch.float32, False, metric="hessian").key not in (soft.key, hess.key)
    n = jit.stats["traced"]
    assert n == traced + 3
    assert jit.compile_rmhmc(fn, ex, torch.float32, True, metric="hessian") is hess and jit.compile_rmhmc(fn, ex, torch.float32, True) is soft
    assert jit.stats["traced"] == n
    with pytest.raises(ValueError):
        jit.compile_rmhmc(fn, ex, torch.float32, True, metric="jacobian_diag")
    with pytest.raises(jit.Unsupported, match="D <= 16"):
        jit.compile_rmhmc(logcosh_logp(*target(17)), torch.ones(17), torch.float32, True, metric="hessian")
    tr = trace_callback(funnel, torch.ones(11, dtype=torch.float64))
    with_metric = runtime.derivs_generated_source(tr, torch.float32, True, "softabs")
    assert with_metric.replace("#define HTA_CB_METRIC HTA_CB_METRIC_SOFTABS\n", "") == runtime.derivs_generated_source(tr, torch.float32, True)
    assert "by reverse mode" not in with_metric


def test_an_unknown_metric_in_the_include_does_not_compile():
    """The skeleton takes its metric from HTA_CB_METRIC of the generated include: a value that is neither metric's is an #error whose
    message names the accepted ones - and so is a name that is no macro at all, which the preprocessor alone would read as 0."""
    tr = trace_callback(logcosh_logp(*target(2)), torch.ones(2, dtype=torch.float64))
    src = runtime.derivs_generated_source(tr, torch.float32, True, "hessian")
    line = "#define HTA_CB_METRIC HTA_CB_METRIC_HESSIAN\n"
    assert src.count(line) == 1
    for value in ("7", "HTA_CB_METRIC_FISHER"):
        with pytest.raises(runtime.CompileError) as e:
            runtime.compile_source(src.replace(line, "#define HTA_CB_METRIC %s\n" % value), runtime.SKELETON_RMHMC)
        assert "HTA_CB_METRIC_SOFTABS" in e.value.log and "HTA_CB_METRIC_HESSIAN" in e.value.log, e.value.log


@pytest.mark.parametrize("D", [2, 5, 11, 16])
def test_the_contraction_by_reverse_mode_equals_the_oracle(D):
    """third_contract as the gradient of the one scalar <Hessian(theta), M> (runtime.contracted_third; M enters through extra inputs
    of the graph): the oracle's c_k = sum_ij (d_k d_i d_j log p) M_ij to rounding.  The Metric.HESSIAN include takes this form; the
    soft-abs one takes it where the entry-by-entry form is beyond MAX_DERIV_NODES (log-cosh from D = 9 on: 21 627 operations)."""
    P, A = target(D)
    tr = trace_callback(logcosh_logp(P, A), torch.ones(D, dtype=torch.float64))
    g = tr.graph
    c = runtime.contracted_third(g, [g.grad(gi) for gi in tr.grad()])
    rng = np.random.default_rng(0)
    th = rng.standard_normal((5, D)); M = rng.standard_normal((5, D, D)); M = M + M.transpose(0, 2, 1)
    m = np.stack([M[:, i, j] * (1 if i == j else 2) for i in range(D) for j in range(i + 1)], -1)       # M_ii | M_ij + M_ji
    got = g.evaluate(c, np.concatenate([th, m], -1), np.float64)
    want = O.LogCoshTarget(P, A).third_contract(th, M)
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-11 * np.abs(want).max())
    assert "by reverse mode" in runtime.derivs_generated_source(tr, torch.float64, True, "hessian")
    assert ("by reverse mode" in runtime.derivs_generated_source(tr, torch.float64, True, "softabs")) == (D >= 11)


def test_oracle_guard():
    """The cases of test_hessian_kernel_vs_oracle on the CPU oracle, float32 against float64: no Metropolis decision differs and the
    rows differ by at most a quarter of the float32 band (5e-3) - so the 10 % of chains the GPU test lets outside the band cannot
    hide an error of the kernel behind decisions the oracle itself would flip."""
    worst = 0.0
    for C, D, jitter, burn in CASES:
        P, A = target(D)
        o = O.LogCoshTarget(P, A)
        res = {}
        for dt in (np.float32, np.float64):
            th0 = (0.4 * O.philox_normals(SEED, OFF + np.arange(C), 0, D, O.PURPOSE_INIT, dtype=np.float64)).astype(dt)
            ref, info = O.sample_rmhmc_explicit(o, th0, N, L, EPS, OMEGA, 1.0, burn, jitter, O.PhiloxDraws(SEED, OFF + np.arange(C), dt), "hessian")
            res[dt] = (np.stack(ref).astype(np.float64), np.stack(info["accept"]))
        flips = int((res[np.float32][1] != res[np.float64][1]).sum())
        dist = float(np.abs(res[np.float32][0] - res[np.float64][0]).max())
        print("C=%d D=%d jitter=%s burn=%d: %d flipped decisions, distance %.3g, acceptance %.2f" % (C, D, jitter, burn, flips, dist, res[np.float64][1].mean()))
        assert flips == 0 and np.isfinite(res[np.float64][0]).all()
        worst = max(worst, dist)
    assert worst <= 0.25 * 5e-3, worst
