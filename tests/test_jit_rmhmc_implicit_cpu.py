"""CPU half of the compiled implicit-RMHMC trajectory kernel (csrc/jit/rmhmc_implicit_callback.hip.in over rmhmc_metric_softabs.inc /
rmhmc_metric_hessian.inc): the skeleton builds for gfx950 through hipRTC for both metrics (no GPU needed) around the generated include
of the explicit kernel, from the same trace; the argument block has one layout in C and in ctypes; the entry point rejects bad
arguments before any launch; and the oracle itself decides the cases of tests/test_gpu_jit_rmhmc_implicit.py in float32 as in float64,
with chains that need different numbers of fixed-point iterations.  This file also holds the cases both halves run.
"""
import ctypes
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import hmc_oracle as O
from hamiltorch_amd import _abi, jit
from hamiltorch_amd.jit import runtime
from hamiltorch_amd.jit.trace import trace_callback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
NP = {torch.float32: np.float32, torch.float64: np.float64}
SEED, OFF, C, N, L, MAX_IT = 99, 7, 70, 5, 2, 12
HL2P = 0.9189385332046727
FUNNEL_SCALES = np.array([0.5, 1.0, 1.7, 2.4, 3.3, 0.8, 1.2, 2.0, 2.9, 0.6])


class Case:
    """One run of sample(RMHMC, IMPLICIT): `kind` "logcosh" (Metric.HESSIAN, eps 0.4) | "funnel" (soft-abs, eps 0.06); thr per dtype."""

    def __init__(self, kind, D, jitter, burn, thr64, thr32, alpha=1.0, max_it=MAX_IT, C=C):
        self.kind, self.D, self.jitter, self.burn, self.alpha, self.max_it, self.C = kind, D, jitter, burn, alpha, max_it, C
        self.thr = {np.float64: thr64, np.float32: thr32}
        self.metric = "hessian" if kind == "logcosh" else "softabs"
        self.eps = 0.4 if kind == "logcosh" else 0.06

    def __repr__(self):
        return "%s-D%d-jit%s-burn%d-a%g-it%d-C%d" % (self.kind, self.D, self.jitter, self.burn, self.alpha, self.max_it, self.C)

    def oracle_target(self):
        return O.LogCoshTarget(*target(self.D)) if self.kind == "logcosh" else O.FunnelTarget(self.D, FUNNEL_SCALES[:self.D - 1])

    def callable(self):
        return logcosh_logp(*target(self.D)) if self.kind == "logcosh" else scaled_funnel(FUNNEL_SCALES[:self.D - 1])

    def start(self, dt, chains=None):
        ids = np.arange(self.C) if chains is None else np.asarray(chains)
        return (0.4 * O.philox_normals(SEED, OFF + ids, 0, self.D, O.PURPOSE_INIT, dtype=np.float64)).astype(dt)

    def oracle(self, dt, chains=None, target_=None, **over):
        """O.sample_rmhmc_implicit on the chains' own Philox streams (keyed by chain id): (rows [S, C, D], info)."""
        ids = np.arange(self.C) if chains is None else np.asarray(chains)
        kw = dict(thr=self.thr[dt], max_it=self.max_it, N=N, L=L)
        kw.update(over)
        with np.errstate(all="ignore"):
            ref, info = O.sample_rmhmc_implicit(target_ or self.oracle_target(), self.start(dt, chains), kw["N"], kw["L"], self.eps, self.alpha,
                                                kw["thr"], kw["max_it"], self.burn, self.jitter, O.PhiloxDraws(SEED, OFF + ids, dt), self.metric)
        return np.stack(ref), info


# (D, jitter, burn, thr64, thr32): thresholds at which the chains of a case leave the loops at different iterations
LOGCOSH = [Case("logcosh", 5, None, 2, 1e-12, 1e-9), Case("logcosh", 8, None, -1, 1e-14, 1e-9), Case("logcosh", 16, None, 0, 1e-12, 1e-9),
           Case("logcosh", 5, 1e-3, 0, 1e-7, 1e-7), Case("logcosh", 8, 1e-2, 0, 1e-5, 1e-5), Case("logcosh", 2, 1e-3, 0, 1e-8, 1e-8)]
LOGCOSH_D1 = Case("logcosh", 1, None, 0, 1e-18, 1e-9, max_it=8)
FUNNEL = [Case("funnel", 5, None, 0, 1e-12, 1e-9, alpha=1e6), Case("funnel", 6, 1e-2, 0, 1e-6, 1e-6, alpha=1.0),
          Case("funnel", 11, 1e-3, 0, 1e-8, 1e-8, alpha=1.0), Case("funnel", 3, None, 0, 1e-12, 1e-9, alpha=0.7)]
ONE_CHAIN = [Case("logcosh", 5, 1e-3, 0, 1e-7, 1e-7, C=1), Case("funnel", 5, None, 0, 1e-12, 1e-9, alpha=1e6, C=1)]
CASES = LOGCOSH + [LOGCOSH_D1] + FUNNEL + ONE_CHAIN


def target(D):
    """The log-cosh target of tests/test_gpu_jit_rmhmc_hessian.py: default_rng(2) draws Q first, then A."""
    rng = np.random.default_rng(2)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    P = (Q * np.linspace(0.5, 2.0, D)) @ Q.T
    P = 0.5 * (P + P.T)
    return P, 0.6 * rng.standard_normal((D + 2, D))


def logcosh_logp(P, A, sign=-1.0):
    def f(w):
        Pt = torch.as_tensor(P, dtype=w.dtype, device=w.device); At = torch.as_tensor(A, dtype=w.dtype, device=w.device)
        return -0.5 * torch.dot(w, torch.mv(Pt, w)) + sign * torch.log(torch.cosh(torch.mv(At, w))).sum()
    return f


def scaled_funnel(scales):
    """The scaled funnel of tests/test_gpu_jit.py (oracle.FunnelTarget(D, scales))."""
    def f(w):
        s = torch.as_tensor(scales, dtype=w.dtype, device=w.device)
        v, x = w[0], w[1:]
        return -v * v / 18.0 - 1.0986122886681098 - HL2P + (-0.5 * torch.exp(v) * (x * x / s).sum() + 0.5 * x.numel() * v
                                                             - x.numel() * HL2P - 0.5 * torch.log(s).sum())
    return f


class Counting:
    """An oracle target that counts its neg_hessian calls: one per metric evaluation."""

    def __init__(self, inner):
        self._inner, self.calls = inner, 0

    def neg_hessian(self, t):
        self.calls += 1
        return self._inner.neg_hessian(t)

    def __getattr__(self, name):
        return getattr(self._inner, name)


_counts = {}


def oracle_iterations(case, dt, chain):
    """Fixed-point iterations chain `chain` executes in a one-chain oracle run (Philox streams are keyed by chain id, the loops of a
    one-chain batch end with the chain): metric evaluations - N (3 + 2 L), the gibbs / H_old / H_new and g0 / final-kick evaluations."""
    key = (repr(case), dt, chain)
    if key not in _counts:
        t = Counting(case.oracle_target())
        case.oracle(dt, [chain], t)
        _counts[key] = t.calls - N * (3 + 2 * L)
    return _counts[key]


def _symbols(blob, tmp_path):
    p = tmp_path / "cb.co"
    p.write_bytes(blob)
    sym = subprocess.run([READELF, "-s", str(p)], capture_output=True, text=True).stdout
    notes = subprocess.run([READELF, "--notes", str(p)], capture_output=True, text=True).stdout
    regs = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", notes)}
    return sym, regs


def _header_constant(name):
    text = open(os.path.join(ROOT, "hamiltorch_amd", "csrc", "jit", "jit_args.h")).read()
    return int(re.search(r"#define %s (\w+)" % name, text).group(1), 0)


def built(fn, D, dtype, jitter, metric, tmp_path):
    tr = trace_callback(fn, torch.ones(D, dtype=torch.float64))
    src = runtime.derivs_generated_source(tr, dtype, jitter, metric)
    key, blob = runtime.compile_source(src, runtime.SKELETON_RMHMC_IMPLICIT)
    return (blob,) + _symbols(blob, tmp_path)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("metric,D", [("hessian", 1), ("hessian", 5), ("hessian", 16), ("softabs", 3), ("softabs", 5)])
def test_the_skeleton_builds_for_both_metrics(metric, D, dtype, tmp_path):
    """gfx950 code objects of the implicit skeleton, jitter off and on: the kernel of the metric (and not the explicit one, whose name the
    metric's file defines), and an info block {magic, D, sizeof(T), jitter, kernel set} of the new sets."""
    name = {"hessian": "hta_cb_rmhmc_imp_hess_kernel", "softabs": "hta_cb_rmhmc_imp_kernel"}[metric]
    kset = _header_constant({"hessian": "HTA_CB_SET_RMHMC_IMP_HESS", "softabs": "HTA_CB_SET_RMHMC_IMP"}[metric])
    assert (_header_constant("HTA_CB_SET_RMHMC_IMP"), _header_constant("HTA_CB_SET_RMHMC_IMP_HESS")) == (8, 9)
    fn = logcosh_logp(*target(D)) if metric == "hessian" else scaled_funnel(FUNNEL_SCALES[:D - 1])
    item = 4 if dtype == torch.float32 else 8
    for jitter in (False, True):
        blob, sym, regs = built(fn, D, dtype, jitter, metric, tmp_path)
        names = set(re.findall(r"\b(hta_cb_\w+)\b", sym))
        assert name in names and "hta_cb_info" in names, names
        assert not names & {"hta_cb_rmhmc_kernel", "hta_cb_rmhmc_hess_kernel"}, names
        assert (name == "hta_cb_rmhmc_imp_kernel") == ("hta_cb_rmhmc_imp_hess_kernel" not in names)
        assert struct.pack("<5i", _header_constant("HTA_CB_MAGIC"), D, item, int(jitter), kset) in blob
        print("%s D=%d %s jitter=%d: %s" % (metric, D, runtime.dtype_name(dtype), jitter, regs))


def test_one_trace_serves_both_integrators():
    """compile_rmhmc(integrator="implicit") goes through the cache entry of the explicit route: one trace, one generated include, two
    modules - in either order - and each is handed out again without a new trace or a new build."""
    fn, ex = logcosh_logp(*target(3)), torch.ones(3, dtype=torch.float32)
    traced, hits = jit.stats["traced"], jit.stats["trace_hits"]
    imp = jit.compile_rmhmc(fn, ex, torch.float32, True, metric="hessian", integrator="implicit")
    assert jit.stats["traced"] == traced + 1
    exp = jit.compile_rmhmc(fn, ex, torch.float32, True, metric="hessian")
    assert jit.stats["traced"] == traced + 1 and jit.stats["trace_hits"] == hits + 1          # served from the same trace
    assert exp.skeleton == runtime.SKELETON_RMHMC and exp.implicit() is imp and imp.key != exp.key and imp.blob != exp.blob
    assert b"hta_cb_rmhmc_imp_hess_kernel" in imp.blob and b"hta_cb_rmhmc_imp_hess_kernel" not in exp.blob
    compiled = runtime.stats["compiled"]
    assert jit.compile_rmhmc(fn, ex, torch.float32, True, metric="hessian", integrator="implicit") is imp
    assert jit.stats["traced"] == traced + 1 and jit.stats["trace_hits"] == hits + 2 and runtime.stats["compiled"] == compiled
    soft = jit.compile_rmhmc(fn, ex, torch.float32, True, integrator="implicit")               # the metric stays part of the key
    assert soft is not imp and b"hta_cb_rmhmc_imp_kernel" in soft.blob and jit.stats["traced"] == traced + 2
    with pytest.raises(ValueError):
        jit.compile_rmhmc(fn, ex, torch.float32, True, integrator="s3")
    with pytest.raises(jit.Unsupported, match="D <= 16"):
        jit.compile_rmhmc(logcosh_logp(*target(17)), torch.ones(17), torch.float32, True, metric="hessian", integrator="implicit")


def test_the_argument_block_has_one_layout(tmp_path):
    """HtaCbRmhmcImpArgs in ctypes against the C compiler's sizeof / offsetof of csrc/jit/jit_args.h; the explicit block is unchanged."""
    fields = [f for f, _ in _abi.HtaCbRmhmcImpArgs._fields_]
    exp = [f for f, _ in _abi.HtaCbRmhmcArgs._fields_]
    assert [f for f in fields if f not in ("iters", "thr", "max_it")] == [f for f in exp if f != "omega"]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "jit_args.h"', 'int main(void) {',
             '  printf("%zu %zu\\n", sizeof(HtaCbRmhmcImpArgs), sizeof(HtaCbRmhmcArgs));']
    lines += ['  printf("%s %%zu\\n", offsetof(HtaCbRmhmcImpArgs, %s));' % (f, f) for f in fields]
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "hamiltorch_amd", "csrc", "jit"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0].split() == [str(ctypes.sizeof(_abi.HtaCbRmhmcImpArgs)), str(ctypes.sizeof(_abi.HtaCbRmhmcArgs))] == ["152", "136"]
    got = dict(ln.split() for ln in out[1:] if ln)
    assert got == {f: str(getattr(_abi.HtaCbRmhmcImpArgs, f).offset) for f in fields}


def test_the_entry_point_rejects_bad_arguments_before_any_launch():
    """hta_jit_rmhmc_implicit_sample without a GPU (its checks of the argument block and the workspace come before the module's, which
    needs a device): max_it < 0, a NaN thr, a short workspace, a NULL module - each with its own message, nothing dereferenced."""
    lib = _abi.load()
    D, C_ = 5, 70
    need = lib.hta_jit_rmhmc_workspace_bytes(C_, D, 8)
    assert need == C_ * 8
    host = (ctypes.c_char * 64)()                      # stands for the device buffers: the checks look at the pointers only

    def call(ws_bytes=need, **over):
        a = _abi.HtaCbRmhmcImpArgs()
        a.cur = a.init = a.reject_count = ctypes.addressof(host)
        a.C, a.eps, a.thr, a.L, a.n_traj, a.max_it = C_, 0.1, 1e-5, 2, 1, 6
        for k, v in over.items():
            setattr(a, k, v)
        rc = lib.hta_jit_rmhmc_implicit_sample(None, ctypes.byref(a), D, 8, 0, ctypes.addressof(host), ws_bytes, None)
        return rc, _abi.last_error()

    rc, msg = call(max_it=-1)
    assert rc != 0 and "max_it = -1" in msg, msg
    rc, msg = call(thr=float("nan"))
    assert rc != 0 and "thr is NaN" in msg, msg
    rc, msg = call(ws_bytes=need - 1)
    assert rc != 0 and "workspace of %d bytes, %d needed" % (need - 1, need) in msg, msg
    rc, msg = call(C=0)
    assert rc != 0 and "bad arguments" in msg, msg
    rc, msg = call()
    assert rc != 0 and "hta_jit_rmhmc_implicit_sample: module is NULL" in msg, msg
    rc, msg = call(max_it=0, thr=0.0)                  # both legal: the module is what is missing
    assert rc != 0 and "module is NULL" in msg, msg


@pytest.fixture(scope="module")
def oracle_pairs():
    """(float32 rows, float64 rows, chains with a flipped decision) of every case on the CPU oracle: the same streams and the same
    threshold (the float32 one), so that the number format is all that differs."""
    out = {}
    for case in CASES:
        r32, i32 = case.oracle(np.float32)
        r64, i64 = case.oracle(np.float64, thr=case.thr[np.float32])
        flips = (np.stack(i32["accept"]) != np.stack(i64["accept"])).any(axis=0)
        out[repr(case)] = (r32.astype(np.float64), r64, flips)
    return out


def test_oracle_guard(oracle_pairs):
    """The cases of test_implicit_kernel_vs_oracle on the CPU oracle, float32 against float64.  Log-cosh under Metric.HESSIAN: no chain
    flips a decision, rows within 1e-6.  The funnel under soft-abs: at alpha = 1e6 (|lambda| itself: the map has a kink) a few of the 70
    chains flip a decision - at most 3, half of the 7 the GPU test lets outside its band, so that as many again are left to the
    kernel's own rounding; the other cases flip none and stay within 1e-6 like the log-cosh ones (measured: 1.7e-7 to 4.1e-7), a
    5000th of the float32 band.  So the 10 % the GPU test allows cannot hide an error of
    the kernel behind decisions the oracle itself would flip."""
    for case in CASES:
        r32, r64, flips = oracle_pairs[repr(case)]
        dist = float(np.abs(r32 - r64)[:, ~flips].max()) if (~flips).any() else 0.0
        print("%r: %d of %d chains flip a decision, distance of the others %.3g" % (case, flips.sum(), case.C, dist))
        assert np.isfinite(r64).all()
        if case.kind == "logcosh":
            assert flips.sum() == 0 and dist <= 1e-6, (case, flips.sum(), dist)
        elif case.alpha == 1e6 and case.C == C:
            assert flips.sum() <= 3, (case, flips.sum())
        else:
            assert flips.sum() == 0 and dist <= 1e-6, (case, flips.sum(), dist)


@pytest.mark.parametrize("case", LOGCOSH + [LOGCOSH_D1] + FUNNEL, ids=repr)
def test_oracle_guard_iteration_spread(case):
    """The chains of a case need different numbers of fixed-point iterations (one-chain oracle runs of the first 12 chains, float64):
    a kernel that ran every loop to the wave's last chain - or to max_it - and let the finished chains go on taking updates would not
    reproduce them.  No chain runs every loop to max_it."""
    counts = [oracle_iterations(case, np.float64, c) for c in range(12)]
    print("%r: iterations of chains 0 .. 11: %s of %d" % (case, counts, N * L * 2 * case.max_it))
    assert len(set(counts)) >= 2, counts
    assert max(counts) < N * L * 2 * case.max_it and min(counts) >= N * L * 2


def test_resources_are_recorded(tmp_path):
    """Registers, spills and scratch of the float32 D = 8 Metric.HESSIAN and D = 5 soft-abs code objects (jitter on) are read from the
    code objects' notes, and profiles/r14a_rmhmc_implicit.json (tools/jit_rmhmc_implicit_rate.py resources) holds a record of the same
    counts.  No bound and no equality: the explicit soft-abs kernel already spills by design, and the counts move with the compiler."""
    rec = json.load(open(os.path.join(ROOT, "profiles", "r14a_rmhmc_implicit.json")))["resources"]
    for name, metric, D, fn in (("hessian_D8_f32", "hessian", 8, logcosh_logp(*target(8))),
                                ("softabs_D5_f32", "softabs", 5, scaled_funnel(FUNNEL_SCALES[:4]))):
        _, _, regs = built(fn, D, torch.float32, True, metric, tmp_path)
        print(name, regs)
        assert set(rec[name]) == set(regs) and all(isinstance(v, int) for v in rec[name].values()), rec[name]
