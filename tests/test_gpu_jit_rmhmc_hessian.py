"""GPU parity of the compiled explicit-RMHMC trajectory kernel for Metric.HESSIAN (csrc/jit/rmhmc_callback.hip.in with rmhmc_metric_hessian.inc,
hta_cb_rmhmc_hess_kernel): sample(sampler=RMHMC, integrator=EXPLICIT, metric=HESSIAN) on a general log-concave callable, one chain
per lane, against the oracle on the same Philox streams (chain by chain), against the launch-per-evaluation route of the same
library (HAMILTORCH_AMD_JIT=0), cut into launches, on a metric that is not positive definite, and through the switches.  The route
is asserted in every run.
"""
import numpy as np
import pytest
import torch

import hmc_oracle as O

pytestmark = pytest.mark.gpu
NP = {torch.float32: np.float32, torch.float64: np.float64}
N, L, EPS, OMEGA, SEED, OFF = 6, 3, 0.4, 10.0, 99, 7
# (C, D, jitter, burn): D = 1 and the register limit D = 16, a partial wave beyond one block, one chain alone, burn-in on and off
CASES = [(70, 1, None, 0), (70, 2, 1e-3, 0), (70, 5, None, 2), (70, 8, 1e-2, -1), (70, 11, 1e-3, 0), (70, 16, 1e-2, 2), (1, 5, 1e-3, 0)]


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


def logcosh_logp(P, A, sign=-1.0):
    """-1/2 w^T P w - sum log cosh(A w) (oracle.LogCoshTarget); sign = +1: the likelihood term with the other sign."""
    def f(w):
        Pt = torch.as_tensor(P, dtype=w.dtype, device=w.device); At = torch.as_tensor(A, dtype=w.dtype, device=w.device)
        return -0.5 * torch.dot(w, torch.mv(Pt, w)) + sign * torch.log(torch.cosh(torch.mv(At, w))).sum()
    return f


def target(D):
    rng = np.random.default_rng(2)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    P = (Q * np.linspace(0.5, 2.0, D)) @ Q.T
    P = 0.5 * (P + P.T)
    A = 0.6 * rng.standard_normal((D + 2, D))
    return P, A


def start(C, D, dtype):
    return (0.4 * O.philox_normals(SEED, OFF + np.arange(C), 0, D, O.PURPOSE_INIT, dtype=np.float64)).astype(NP[dtype])


def run(ht, fn, th0, metric=None, **over):
    kw = dict(num_samples=N, num_steps_per_sample=L, step_size=EPS, explicit_binding_const=OMEGA, sampler=ht.Sampler.RMHMC,
              integrator=ht.Integrator.EXPLICIT, metric=metric or ht.Metric.HESSIAN, debug=2, verbose=False, seed=SEED, chain_offset=OFF)
    kw.update(over)
    out, acc = ht.sample(fn, th0, **kw)
    return torch.stack(list(out)), acc


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-7), (torch.float32, 5e-3)])
@pytest.mark.parametrize("C,D,jitter,burn", CASES)
def test_hessian_kernel_vs_oracle(ht, dtype, tol, C, D, jitter, burn):
    """Every chain against oracle.sample_rmhmc_explicit(metric="hessian") on the same Philox streams (momentum by chol(G) z, 8 jitter
    sub-streams per step in the reference's order, Q1 / Q2 / Q4), with the tolerances of test_fused_rmhmc_kernel_vs_oracle: float64 1e-7,
    float32 5e-3, at most 10 % of the chains outside the band, the acceptance rates of the others equal.  On the CPU oracle, float32
    against float64, no chain of these cases flips a decision and the largest distance is 5.7e-6
    (tests/test_jit_rmhmc_hessian_cpu.py::test_oracle_guard); 2 to 58 chains of every 70-chain case reject trajectory burn + 1."""
    P, A = target(D)
    th0 = start(C, D, dtype)
    out, acc = run(ht, logcosh_logp(P, A), tt(th0, dtype), burn=burn, jitter=jitter)
    assert "hta_cb_rmhmc_hess_kernel<D=%d" % D in route(), route()
    ref, info = O.sample_rmhmc_explicit(O.LogCoshTarget(P, A), th0, N, L, EPS, OMEGA, 1.0, burn, jitter,
                                        O.PhiloxDraws(SEED, OFF + np.arange(C), NP[dtype]), "hessian")
    got, want = out.cpu().numpy(), np.stack(ref)
    assert got.shape == want.shape
    err = np.abs(got - want).max(axis=(0, 2))
    bad = ~(err <= tol)
    print("C=%d D=%d %s: max err %.3g, %d chains outside, acceptance %.2f" % (C, D, dtype, np.nanmax(err), bad.sum(), info["acc_rate"].mean()))
    assert bad.mean() <= 0.1, "%d of %d chains differ, max err %.3g" % (bad.sum(), C, np.nanmax(err))
    np.testing.assert_allclose(acc.cpu().numpy()[~bad], info["acc_rate"][~bad], atol=1e-12)


def test_hessian_kernel_equals_the_launch_sequence(ht, monkeypatch):
    """The same run in the compiled kernel and on the launch-per-evaluation route (HAMILTORCH_AMD_JIT=0: torch.func derivatives +
    hta_metric_eval): D = 8, float64, jitter 1e-3, 40 chains; at most 10 % of the chains differ by more than 1e-6."""
    P, A = target(8)
    fn, th0 = logcosh_logp(P, A), tt(start(40, 8, torch.float64), torch.float64)
    a, _ = run(ht, fn, th0, jitter=1e-3)
    assert "hta_cb_rmhmc_hess_kernel<D=8,f64,jitter=1" in route(), route()
    monkeypatch.setenv("HAMILTORCH_AMD_JIT", "0")
    b, _ = run(ht, fn, th0, jitter=1e-3)
    assert "hta_cb_rmhmc" not in route(), route()
    err = (a - b).abs().amax(dim=(0, 2))
    assert float((err > 1e-6).double().mean()) <= 0.1, float(err.max())


def test_a_run_cut_into_launches_is_bit_identical(ht, capsys):
    """verbose=True cuts the run into launches of ceil(N / 20) = 1 trajectory (traj_offset 0 .. 5, the Q2 reset of trajectory burn + 1
    in a launch of its own); the rows and the rejection counts are those of the one-launch run bit for bit."""
    P, A = target(5)
    fn, th0 = logcosh_logp(P, A), tt(start(70, 5, torch.float32), torch.float32)
    a, acc_a = run(ht, fn, th0, jitter=1e-3, burn=2)
    assert "hta_cb_rmhmc_hess_kernel<D=5,f32,jitter=1" in route(), route()
    b, acc_b = run(ht, fn, th0, jitter=1e-3, burn=2, verbose=True)
    assert "hta_cb_rmhmc_hess_kernel<D=5,f32,jitter=1" in route(), route()
    capsys.readouterr()
    assert torch.equal(a, b) and torch.equal(acc_a, acc_b)
    assert 0 < float(acc_a.mean()) < 1


def test_a_metric_that_is_not_positive_definite_rejects(ht, monkeypatch):
    """-1/2 w^T P w + sum log cosh(a_i . w) at D = 4: -Hessian = P - sum sech^2(a_i . w) a_i a_i^T is indefinite around the origin (one
    long a_i along P's softest direction) and tends to P far along it.  The reference's `cholesky` raises there; the kernel's factor is
    NaN through plain arithmetic, the energies are non-finite, every proposal is rejected: chains started in the indefinite region stay
    on their start for the whole run, the others move, every stored row is finite - and the run agrees with the launch sequence."""
    D, C = 4, 64
    P, _ = target(D)
    w, V = np.linalg.eigh(P)
    A = np.stack([1.5 * V[:, 0], 0.3 * V[:, 1]])                     # P - A^T A at the origin: 0.5 - 2.25 along V[:, 0]
    nh = lambda th: P - np.einsum("ci,ia,ib->cab", 1.0 / np.cosh(th @ A.T) ** 2, A, A)     # noqa: E731
    rng = np.random.default_rng(5)
    th0 = 0.05 * rng.standard_normal((C, D))
    th0[C // 2:] += 3.0 * V[:, 0]                                     # sech^2(4.5) = 5e-4: -Hessian is P to three digits
    lam = np.linalg.eigvalsh(nh(th0))[:, 0]
    indef = np.arange(C) < C // 2
    assert (lam[indef] < -0.1).all() and (lam[~indef] > 0.1).all(), lam
    fn, t0 = logcosh_logp(P, A, sign=1.0), tt(th0, torch.float64)
    ti = torch.from_numpy(indef).to(dev())
    a, acc = run(ht, fn, t0)
    assert "hta_cb_rmhmc_hess_kernel<D=4,f64,jitter=0" in route(), route()
    assert torch.isfinite(a).all()
    assert torch.equal(a[:, ti], t0[ti].expand(a.shape[0], -1, -1)) and float(acc[ti].abs().max()) == 0.0     # rejected == N
    assert float(acc[~ti].max()) > 0.0                                # (the other half is sampled)
    monkeypatch.setenv("HAMILTORCH_AMD_JIT", "0")
    b, _ = run(ht, fn, t0)
    assert "hta_cb_rmhmc" not in route(), route()
    err = (a - b).abs().amax(dim=(0, 2))
    print("indefinite starts: max difference to the launch sequence %.3g, the others %.3g" % (float(err[ti].max()), float(err[~ti].max())))
    assert float((err > 1e-6).double().mean()) <= 0.1, float(err.max())


def test_softabs_still_takes_the_softabs_kernel(ht, monkeypatch):
    """The metric chooses the kernel and the switches are those of the soft-abs route: the same callable under Metric.SOFTABS runs
    hta_cb_rmhmc_kernel; native=False and HAMILTORCH_AMD_JIT=0 keep the launch sequence."""
    P, A = target(5)
    fn, th0 = logcosh_logp(P, A), tt(start(12, 5, torch.float64), torch.float64)
    a, _ = run(ht, fn, th0, jitter=1e-3)
    assert "hta_cb_rmhmc_hess_kernel<D=5" in route(), route()
    run(ht, fn, th0, jitter=1e-3, metric=ht.Metric.SOFTABS, softabs_const=1e6)
    assert "hta_cb_rmhmc_kernel<D=5,f64,jitter=1" in route(), route()
    b, _ = run(ht, fn, th0, jitter=1e-3, native=False)
    assert "hta_cb_rmhmc" not in route(), route()
    assert float(((a - b).abs().amax(dim=(0, 2)) > 1e-6).double().mean()) <= 0.1
    monkeypatch.setenv("HAMILTORCH_AMD_JIT", "0")
    run(ht, fn, th0, jitter=1e-3)
    assert "hta_cb_rmhmc" not in route(), route()


def test_beyond_the_register_limit_the_run_falls_back_and_says_why(ht):
    """D = 17 under Metric.HESSIAN: the compiled route declines with the D limit in hta_last_route(), sample() runs the launch sequence."""
    from hamiltorch_amd import _abi, jit, rmhmc
    P, A = target(17)
    fn, th0 = logcosh_logp(P, A), tt(start(4, 17, torch.float64), torch.float64)
    assert rmhmc._sample_explicit_compiled(fn, th0, 2, 1, 0.1, 0, None, None, OMEGA, _abi.METRIC_HESSIAN, SEED, 0, False) is None
    assert "not compiled" in route() and "D = 17" in route() and "D <= 16" in jit.last_reason(), route()
    out, _ = run(ht, fn, th0, num_samples=2, num_steps_per_sample=1, step_size=0.1)
    assert "hta_cb_rmhmc" not in route() and torch.isfinite(out).all(), route()
