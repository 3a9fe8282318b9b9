"""GPU parity of the compiled implicit-RMHMC trajectory kernel (csrc/jit/rmhmc_implicit_callback.hip.in: hta_cb_rmhmc_imp_kernel for the
soft-abs metric, hta_cb_rmhmc_imp_hess_kernel for Metric.HESSIAN): sample(sampler=RMHMC, integrator=IMPLICIT) on a general callable, one
chain per lane, against the oracle on the same Philox streams (chain by chain, and iteration count by iteration count), at the edges of
the fixed-point rule, at sample()'s defaults, against the launch sequence of the same library (HAMILTORCH_AMD_JIT_IMPLICIT=0), cut into
launches, on a metric that is not positive definite, and through the switches.  The route is asserted in every run.  The cases and their
oracle guards are in tests/test_jit_rmhmc_implicit_cpu.py.
"""
import numpy as np
import pytest
import torch

import hmc_oracle as O
from test_jit_rmhmc_implicit_cpu import (CASES, FUNNEL, LOGCOSH, N, L, OFF, SEED, Case, logcosh_logp, oracle_iterations, target)

pytestmark = pytest.mark.gpu
NP = {torch.float32: np.float32, torch.float64: np.float64}
TOL = {torch.float64: 1e-7, torch.float32: 5e-3}
KERNEL = {"hessian": "hta_cb_rmhmc_imp_hess_kernel", "softabs": "hta_cb_rmhmc_imp_kernel"}


@pytest.fixture(scope="module")
def ht():
    import hamiltorch_amd
    assert torch.cuda.is_available()
    return hamiltorch_amd


def dev():
    return torch.device("cuda:0")


def tt(a, dtype):
    return torch.tensor(a, dtype=dtype, device=dev())


def route():
    from hamiltorch_amd import _abi
    return _abi.last_route()


def run(ht, case, dtype, fn=None, th0=None, **over):
    kw = dict(num_samples=N, num_steps_per_sample=L, step_size=case.eps, burn=case.burn, jitter=case.jitter, softabs_const=case.alpha,
              fixed_point_threshold=case.thr[NP[dtype]], fixed_point_max_iterations=case.max_it, sampler=ht.Sampler.RMHMC,
              integrator=ht.Integrator.IMPLICIT, metric=ht.Metric.HESSIAN if case.metric == "hessian" else ht.Metric.SOFTABS,
              debug=2, verbose=False, seed=SEED, chain_offset=OFF)
    kw.update(over)
    out, acc = ht.sample(fn or case.callable(), tt(case.start(NP[dtype]), dtype) if th0 is None else th0, **kw)
    return torch.stack(list(out)), acc


def on_the_kernel(case, dtype):
    want = "%s<D=%d,%s,jitter=%d" % (KERNEL[case.metric], case.D, "f32" if dtype == torch.float32 else "f64", case.jitter is not None)
    assert want in route(), route()


def against_the_oracle(case, dtype, out, acc, what="", **over):
    """Chain by chain: at most 10 % of the chains outside the band, the acceptance rates of the others equal."""
    ref, info = case.oracle(NP[dtype], **over)
    got = out.cpu().numpy()
    assert got.shape == ref.shape
    err = np.abs(got - ref).max(axis=(0, 2))
    bad = ~(err <= TOL[dtype])
    print("%r %s %s: max err %.3g, %d chains outside, acceptance %.2f" % (case, dtype, what, np.nanmax(err), bad.sum(), info["acc_rate"].mean()))
    assert bad.mean() <= 0.1, "%d of %d chains differ, max err %.3g" % (bad.sum(), case.C, np.nanmax(err))
    np.testing.assert_allclose(acc.cpu().numpy()[~bad], info["acc_rate"][~bad], atol=1e-12)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_implicit_kernel_vs_oracle(ht, case, dtype):
    """Every chain against oracle.sample_rmhmc_implicit(..., metric) on the same Philox streams (jitter sub-streams by position), with
    the explicit kernels' tolerances: float64 1e-7, float32 5e-3, at most 10 % of the chains outside the band, the acceptance rates of
    the others equal.  The oracle alone, float32 against float64, flips at most 2 of 70 chains and moves the others by at most 1e-6
    (tests/test_jit_rmhmc_implicit_cpu.py::test_oracle_guard); the chains of a case need different numbers of iterations
    (::test_oracle_guard_iteration_spread)."""
    out, acc = run(ht, case, dtype)
    on_the_kernel(case, dtype)
    against_the_oracle(case, dtype, out, acc)


@pytest.mark.parametrize("case", [LOGCOSH[0], LOGCOSH[4], FUNNEL[1]], ids=repr)
def test_iteration_counts_vs_oracle(ht, case):
    """HtaCbRmhmcImpArgs::iters through runtime.rmhmc_implicit_sample, float64: the fixed-point iterations every chain executed while
    active, over one launch of the whole run.  The first 12 chains and the last 6 (the partial wave) against one-chain oracle runs; at
    most one of the 18 may differ (a diff within rounding of thr)."""
    from hamiltorch_amd import jit
    dt = torch.float64
    th0 = tt(case.start(np.float64), dt)
    comp = jit.compile_rmhmc(case.callable(), th0[0], dt, case.jitter is not None, metric=case.metric, integrator="implicit")
    module = comp.module(th0.device)
    cur, rejected = th0.clone(), torch.zeros(case.C, dtype=torch.int32, device=dev())
    iters = torch.zeros(case.C, dtype=torch.int32, device=dev())
    ws = torch.empty(jit.runtime.rmhmc_workspace_bytes(case.C, case.D, 8), dtype=torch.uint8, device=dev())
    jit.runtime.rmhmc_implicit_sample(module, cur, th0, L, case.eps, case.alpha, case.jitter, case.thr[np.float64], case.max_it, N, 0, case.burn,
                                      SEED, OFF, None, rejected, ws, iters=iters)
    on_the_kernel(case, dt)
    got = iters.cpu().numpy()
    chains = list(range(12)) + list(range(case.C - 6, case.C))
    want = np.array([oracle_iterations(case, np.float64, c) for c in chains])
    print("%r: kernel %s, oracle %s" % (case, got[chains].tolist(), want.tolist()))
    assert (got[chains] != want).sum() <= 1, (got[chains], want)
    assert len(set(got.tolist())) >= 2 and got.max() < N * L * 2 * case.max_it


@pytest.mark.parametrize("what,over", [("max_it=1", dict(max_it=1)), ("max_it=0", dict(max_it=0)), ("thr=1e30", dict(thr=1e30)),
                                       ("thr=0", dict(thr=0.0))])
def test_threshold_edges(ht, what, over):
    """The edges of the fixed-point rule against the oracle, float64, D = 5 Metric.HESSIAN with jitter: one iteration per loop; none
    (the sub-streams of g0, the final kicks and H_new stay where they are); a threshold every chain meets in its first iteration (it
    still takes that iteration's update); and thr = 0, which nobody meets - equal to thr = 1e-300 bit for bit."""
    case, dt = LOGCOSH[3], torch.float64
    kw = dict(fixed_point_max_iterations=over.get("max_it", case.max_it), fixed_point_threshold=over.get("thr", case.thr[np.float64]))
    out, acc = run(ht, case, dt, **kw)
    on_the_kernel(case, dt)
    against_the_oracle(case, dt, out, acc, what, **over)
    if what == "thr=0":
        b, acc_b = run(ht, case, dt, fixed_point_threshold=1e-300)
        on_the_kernel(case, dt)
        assert torch.equal(out, b) and torch.equal(acc, acc_b)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_sample_defaults_exit_early(ht, dtype):
    """sample()'s defaults, fixed_point_max_iterations=1000 and fixed_point_threshold=1e-5 (N = 2, L = 2, D = 5, jitter 1e-3), against
    the oracle: the loops end on the wave-wide vote after a handful of iterations - a kernel that ran all 4000 per trajectory would
    still agree, but not within a test's time."""
    case = Case("logcosh", 5, 1e-3, 0, 1e-5, 1e-5, max_it=1000)
    out, acc = run(ht, case, dtype, num_samples=2)
    on_the_kernel(case, dtype)
    against_the_oracle(case, dtype, out, acc, "defaults", N=2)


@pytest.mark.parametrize("case,C", [(LOGCOSH[4], 40), (Case("funnel", 5, 1e-2, 0, 1e-8, 1e-8, alpha=1.0), 40)], ids=["hessian-D8", "softabs-D5"])
def test_implicit_kernel_equals_the_launch_sequence(ht, monkeypatch, case, C):
    """The same run in the compiled kernel and on the launch sequence of the same library (HAMILTORCH_AMD_JIT_IMPLICIT=0: compiled
    derivatives + hta_metric_eval, one launch per evaluation): float64, 40 chains; at most 10 % of the chains differ by more than 1e-6."""
    dt = torch.float64
    th0 = tt(case.start(np.float64)[:C], dt)
    a, _ = run(ht, case, dt, th0=th0)
    on_the_kernel(case, dt)
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_IMPLICIT", "0")
    b, _ = run(ht, case, dt, th0=th0)
    assert "hta_cb_rmhmc_imp" not in route() and "HAMILTORCH_AMD_JIT_IMPLICIT=0" in route(), route()
    err = (a - b).abs().amax(dim=(0, 2))
    assert float((err > 1e-6).double().mean()) <= 0.1, float(err.max())


def test_a_run_cut_into_launches_is_bit_identical(ht, capsys):
    """verbose=True cuts the run into launches of ceil(N / 20) = 1 trajectory (the Q2 reset of trajectory burn + 1 in a launch of its
    own); the rows and the rejection counts are those of the one-launch run bit for bit."""
    case, dt = Case("logcosh", 5, 1e-3, 2, 1e-7, 1e-7), torch.float32
    a, acc_a = run(ht, case, dt)
    on_the_kernel(case, dt)
    b, acc_b = run(ht, case, dt, verbose=True)
    on_the_kernel(case, dt)
    capsys.readouterr()
    assert torch.equal(a, b) and torch.equal(acc_a, acc_b)
    assert 0 < float(acc_a.mean()) < 1


def test_a_metric_that_is_not_positive_definite_rejects(ht, monkeypatch):
    """The construction of tests/test_gpu_jit_rmhmc_hessian.py: -Hessian indefinite around the origin, P far along its softest
    direction.  The kernel's factor is NaN through plain arithmetic, a non-finite chain stops iterating and its energy rejects it:
    chains started in the indefinite region stay on their start for the whole run, the others move, every stored row is finite - and
    the run agrees with the launch sequence."""
    D, C = 4, 64
    P, _ = target(D)
    w, V = np.linalg.eigh(P)
    A = np.stack([1.5 * V[:, 0], 0.3 * V[:, 1]])
    nh = lambda th: P - np.einsum("ci,ia,ib->cab", 1.0 / np.cosh(th @ A.T) ** 2, A, A)     # noqa: E731
    rng = np.random.default_rng(5)
    th0 = 0.05 * rng.standard_normal((C, D))
    th0[C // 2:] += 3.0 * V[:, 0]
    lam = np.linalg.eigvalsh(nh(th0))[:, 0]
    indef = np.arange(C) < C // 2
    assert (lam[indef] < -0.1).all() and (lam[~indef] > 0.1).all(), lam
    case, dt = Case("logcosh", D, None, 0, 1e-12, 1e-9, C=C), torch.float64
    fn, t0 = logcosh_logp(P, A, sign=1.0), tt(th0, dt)
    ti = torch.from_numpy(indef).to(dev())
    a, acc = run(ht, case, dt, fn=fn, th0=t0)
    on_the_kernel(case, dt)
    assert torch.isfinite(a).all()
    assert torch.equal(a[:, ti], t0[ti].expand(a.shape[0], -1, -1)) and float(acc[ti].abs().max()) == 0.0     # rejected == N
    assert float(acc[~ti].max()) > 0.0
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_IMPLICIT", "0")
    b, _ = run(ht, case, dt, fn=fn, th0=t0)
    assert "hta_cb_rmhmc_imp" not in route(), route()
    err = (a - b).abs().amax(dim=(0, 2))
    print("indefinite starts: max difference to the launch sequence %.3g, the others %.3g" % (float(err[ti].max()), float(err[~ti].max())))
    assert float((err > 1e-6).double().mean()) <= 0.1, float(err.max())


@pytest.mark.parametrize("what", ["D=17", "native=False", "HAMILTORCH_AMD_JIT_IMPLICIT=0", "HAMILTORCH_AMD_JIT=0"])
def test_switches_and_refusals(ht, monkeypatch, what):
    """Each switch - and D = 17, beyond the register limit - keeps the launch sequence and leaves its reason in hta_last_route(); that
    route still passes the oracle comparison (D = 5, Metric.HESSIAN, jitter, float64)."""
    from hamiltorch_amd import _abi, jit, rmhmc
    dt = torch.float64
    if what == "D=17":
        case = Case("logcosh", 17, None, 0, 1e-10, 1e-9, C=4)
        th0 = tt(case.start(np.float64), dt)
        assert rmhmc._sample_implicit_compiled(case.callable(), th0, 2, 1, 0.1, 0, None, None, _abi.METRIC_HESSIAN, 1e-10, 6, SEED, 0, False) is None
        assert "not compiled" in route() and "D = 17" in route() and "D <= 16" in jit.last_reason(), route()
        out, _ = run(ht, case, dt, num_samples=2, num_steps_per_sample=1, step_size=0.1, fixed_point_max_iterations=6)
        assert "hta_cb_rmhmc_imp" not in route() and "D = 17" in route() and torch.isfinite(out).all(), route()
        return
    case, over = LOGCOSH[3], {}
    if what == "native=False":
        over["native"] = False
    else:
        monkeypatch.setenv(*what.split("="))
    out, acc = run(ht, case, dt, **over)
    assert "hta_cb_rmhmc_imp" not in route() and "not compiled: %s)" % what in route(), route()
    against_the_oracle(case, dt, out, acc, what)


def test_bad_arguments_are_rejected_with_a_module(ht):
    """With a loaded module: max_it < 0, a NaN thr and a short workspace raise before anything is launched, and an explicit module is
    not taken for an implicit one."""
    from hamiltorch_amd import _abi, jit
    case, dt = LOGCOSH[3], torch.float64
    th0 = tt(case.start(np.float64), dt)
    fn = case.callable()
    module = jit.compile_rmhmc(fn, th0[0], dt, True, metric="hessian", integrator="implicit").module(th0.device)
    cur, rejected = th0.clone(), torch.zeros(case.C, dtype=torch.int32, device=dev())
    ws = torch.empty(jit.runtime.rmhmc_workspace_bytes(case.C, case.D, 8), dtype=torch.uint8, device=dev())

    def call(module=module, thr=1e-7, max_it=12, ws=ws):
        jit.runtime.rmhmc_implicit_sample(module, cur, th0, L, case.eps, None, case.jitter, thr, max_it, 1, 0, 0, SEED, OFF, None, rejected, ws)

    for kw, msg in ((dict(max_it=-1), "max_it = -1"), (dict(thr=float("nan")), "thr is NaN"), (dict(ws=ws[:-1]), "workspace of"),
                    (dict(module=jit.compile_rmhmc(fn, th0[0], dt, True, metric="hessian").module(th0.device)), "kernel set")):
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    torch.cuda.synchronize()
    assert torch.equal(cur, th0) and int(rejected.abs().max()) == 0
