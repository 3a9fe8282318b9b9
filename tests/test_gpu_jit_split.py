"""GPU parity of the callback compiler for LISTS of callables (hamiltorch_amd/jit/ + csrc/jit/split_callback.hip.in): the split
integrators (Integrator.SPLITTING / SPLITTING_RAND / SPLITTING_KMID) on plain closures, traced, differentiated and built into ONE fused
trajectory kernel - against the oracle on the same Philox streams (chain by chain, the tolerances of tests/test_gpu_jit.py: 2e-4 end to
end in fp32, 1e-9 in fp64, <= 3 % of chains may flip a Metropolis decision at rounding; on this instance the oracle in fp32 against the
oracle in fp64 leaves no chain outside 2e-4, so a failure at the cap is the kernel's), against the torch-evaluated generic route, and
through the fall-back rules.  The route is asserted in every test.
"""
import os

import numpy as np
import pytest
import torch

import hmc_oracle as O

pytestmark = pytest.mark.gpu
NP = {torch.float32: np.float32, torch.float64: np.float64}
D, M, ROWS = 6, 3, 8
KINDS = {"symmetric": "SPLITTING", "rand": "SPLITTING_RAND", "kmid": "SPLITTING_KMID"}


@pytest.fixture(scope="module")
def ht():
    import hamiltorch_amd
    assert torch.cuda.is_available()
    return hamiltorch_amd


def dev():
    return torch.device("cuda:0")


def tt(a, dtype):
    return None if a is None else torch.tensor(a, dtype=dtype, device=dev())


def route():
    from hamiltorch_amd import _abi
    return _abi.last_route()


def rand_spd(D, seed, lo=0.5, hi=1.5):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    P = (Q * np.linspace(lo, hi, D)) @ Q.T
    return 0.5 * (P + P.T)


def masses(D, dtype):
    rng = np.random.default_rng(0)
    return {"none": None, "diag": rng.uniform(0.5, 2.0, D).astype(NP[dtype]), "full": rand_spd(D, 7).astype(NP[dtype])}


def start(C, D, seed, dtype, off=0, scale=0.5):
    return (scale * O.philox_normals(seed, off + np.arange(C), 0, D, O.PURPOSE_INIT, dtype=np.float64)).astype(NP[dtype])


def compare(got, ref, tol, max_bad):
    got = np.stack([g.cpu().numpy() for g in got]); ref = np.stack(ref)
    assert got.shape == ref.shape
    err = np.abs(got - ref).max(axis=(0, 2))
    bad = ~(err <= tol)
    print("chains outside %.1e: %d of %d (largest difference %.3g)" % (tol, bad.sum(), bad.size, np.nanmax(err)))
    assert bad.mean() <= max_bad, "%d of %d chains differ (max err %.3g)" % (bad.sum(), bad.size, np.nanmax(err))
    return bad


# ---- the instance: Bayesian logistic regression, D = 6, 24 rows, M = 3 subsets of 8, prior -(0.5 / M) |w|^2 per subset ------------
def _data():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((M * ROWS, D))
    y = (rng.uniform(size=M * ROWS) > 0.5).astype(np.float64)
    return X, y


_closures = {}


def logistic_closures(dtype):
    """Three plain closures over device tensors (no `_hta_spec`: the native MLP engine declines them).  One list per dtype for the
    module, so that its trace is reused from test to test."""
    if dtype not in _closures:
        X, y = _data()
        fns = []
        for m in range(M):
            A, yy = tt(X[m * ROWS:(m + 1) * ROWS], dtype), tt(y[m * ROWS:(m + 1) * ROWS], dtype)

            def f(w, A=A, yy=yy):
                z = A @ w
                return (yy * z - torch.nn.functional.softplus(z)).sum() - (0.5 / M) * (w * w).sum()
            fns.append(f)
        _closures[dtype] = fns
    return _closures[dtype]


def logistic_oracle(dtype):
    """(logp_fns, grad_fns) of the same three subsets in numpy, in the run's dtype."""
    X, y = _data()
    dt = NP[dtype]
    lf, gf = [], []
    for m in range(M):
        A, yy = X[m * ROWS:(m + 1) * ROWS].astype(dt), y[m * ROWS:(m + 1) * ROWS].astype(dt)
        lf.append(lambda th, A=A, yy=yy: ((th @ A.T) * yy - np.logaddexp(0, th @ A.T)).sum(-1) - dt(0.5 / M) * (th * th).sum(-1))
        gf.append(lambda th, A=A, yy=yy: (yy - 1 / (1 + np.exp(-(th @ A.T)))) @ A - dt(1.0 / M) * th)
    return lf, gf


def oracle_run(dtype, th0, N, L, eps, burn, im, seed, off, kind):
    lf, gf = logistic_oracle(dtype)
    C = th0.shape[0]
    return O.sample_hmc(None, th0, N, L, eps, burn, im, O.PhiloxDraws(seed, off + np.arange(C), NP[dtype]), grad_fns=gf, logp_fns=lf,
                        split_kind=kind)


def integrator(ht, kind):
    return getattr(ht.Integrator, KINDS[kind])


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-4), (torch.float64, 1e-9)], ids=["f32", "f64"])
@pytest.mark.parametrize("C", [256, 1024, 1000])
@pytest.mark.parametrize("burn", [0, 3, -1])
@pytest.mark.parametrize("mass", ["none", "diag", "full"])
@pytest.mark.parametrize("kind", ["symmetric", "rand", "kmid"])
def test_compiled_list_vs_oracle(ht, kind, mass, burn, C, dtype, tol):
    """sample() on a list of plain closures: the fused split kernel, every chain against oracle.sample_hmc(grad_fns=, logp_fns=,
    split_kind=) on the same draws (burn-in bookkeeping, the Q2 reset, mass matrices, a last wave with idle lanes: C = 1000)."""
    N, L, eps, seed, off = 14, 8, 0.1, 777, 5
    th0 = start(C, D, seed, dtype, off)
    im = masses(D, dtype)[mass]
    out, acc = ht.sample(logistic_closures(dtype), tt(th0, dtype), num_samples=N, num_steps_per_sample=L, step_size=eps, burn=burn,
                         inv_mass=tt(im, dtype), integrator=integrator(ht, kind), debug=2, verbose=False, seed=seed, chain_offset=off)
    r = route()
    assert "hta_cb_split_kernel<D=6,M=3,%s,mass=%d,kind=%s," % ("f32" if dtype == torch.float32 else "f64", ["none", "diag", "full"].index(mass), kind) in r, r
    ref, info = oracle_run(dtype, th0, N, L, eps, burn, im, seed, off, kind)
    assert len(out) == len(ref) == N - max(burn, -1)
    bad = compare(out, ref, tol * 5 if mass == "full" else tol, 0.03)
    np.testing.assert_allclose(acc.cpu().numpy()[~bad], info["acc_rate"][~bad], atol=1e-12)
    assert 0.5 < float(acc.mean()) <= 1.0


@pytest.mark.parametrize("kind", ["symmetric", "rand", "kmid"])
def test_compiled_route_equals_generic_route(ht, kind, monkeypatch):
    """The same list on the torch-evaluated generic route (HAMILTORCH_AMD_JIT=0: vmap(grad) per stage + pieces kernels) and compiled:
    float64, the same chains to 1e-8, the same reject counts on the chains that did not flip."""
    C, N, L, eps, seed = 256, 12, 6, 0.3, 31
    fns = logistic_closures(torch.float64)
    th0 = tt(start(C, D, seed, torch.float64), torch.float64)
    kw = dict(num_samples=N, num_steps_per_sample=L, step_size=eps, burn=2, integrator=integrator(ht, kind), debug=2, verbose=False, seed=seed)
    a, acc_a = ht.sample(fns, th0, **kw)
    assert "hta_cb_split_kernel" in route() and "kind=%s" % kind in route(), route()
    monkeypatch.setenv("HAMILTORCH_AMD_JIT", "0")
    b, acc_b = ht.sample(fns, th0, **kw)
    assert "hta_cb_split_kernel" not in route() and "HAMILTORCH_AMD_JIT=0" in route(), route()
    bad = compare(a, [x.cpu().numpy() for x in b], 1e-8, 0.02)
    assert torch.equal(acc_a.cpu()[~bad], acc_b.cpu()[~bad])


def test_rand_orders_differ_between_seeds_and_match_the_oracle(ht):
    """SPLITTING_RAND: one subset order per trajectory from the (seed, trajectory) Philox stream - hta::split_permutation in the kernel,
    util.split_permutation on the host, philox_permutation in the oracle.  Two seeds visit the subsets in different orders; each run
    reproduces the oracle that uses ITS orders (the subsets hold different rows: another order is another trajectory)."""
    C, N, L, eps = 192, 10, 5, 0.2
    dtype = torch.float64
    orders = {}
    for seed in (11, 12):
        orders[seed] = [tuple(O.philox_permutation(seed, n, M)) for n in range(N)]
        assert len(set(orders[seed])) > 1                                        # the order changes from trajectory to trajectory
        th0 = start(C, D, seed, dtype)
        out = ht.sample(logistic_closures(dtype), tt(th0, dtype), num_samples=N, num_steps_per_sample=L, step_size=eps,
                        integrator=ht.Integrator.SPLITTING_RAND, verbose=False, seed=seed)
        assert "hta_cb_split_kernel" in route() and "kind=rand" in route(), route()
        ref, _ = oracle_run(dtype, th0, N, L, eps, 0, None, seed, 0, "rand")
        compare(out, ref, 1e-9, 0.03)
    assert orders[11] != orders[12]
    from hamiltorch_amd import util
    assert [tuple(util.split_permutation(11, n, M)) for n in range(N)] == orders[11]


@pytest.mark.parametrize("kind,eps", [("symmetric", 0.8), ("rand", 0.5), ("kmid", 0.5)])
def test_chunked_runs_are_bit_identical(ht, kind, eps):
    """A run cut into launches (verbose progress: ~20 launches, `resume`) equals the one-launch run bit for bit.  The step size is large
    enough that a good share of proposals is rejected (the oracle's acceptance on this instance: 0.42 / 0.59 / 0.66), so the carried
    log p crosses launch boundaries on both branches; burn = 4 puts the Q2 reset inside the run."""
    fns = logistic_closures(torch.float32)
    th0 = tt(start(200, D, 13, torch.float32), torch.float32)
    kw = dict(num_samples=45, num_steps_per_sample=7, step_size=eps, burn=4, seed=13, integrator=integrator(ht, kind), debug=2)
    one, acc = ht.sample(fns, th0, verbose=False, **kw)
    assert "hta_cb_split_kernel" in route(), route()
    many, acc_m = ht.sample(fns, th0, verbose=True, **kw)
    assert "hta_cb_split_kernel" in route(), route()
    assert torch.equal(torch.stack(list(one)), torch.stack(list(many))) and torch.equal(acc, acc_m)
    assert 0.2 < float(acc.mean()) < 0.9, float(acc.mean())


def test_nuts_on_a_list_adapts_like_the_generic_route(ht):
    """Sampler.HMC_NUTS on a list: one launch per burn-in trajectory with H_old / H_new read back; the final step size within 5 % of the
    generic route's (the bound of test_single_chain_contract_and_nuts)."""
    fns = logistic_closures(torch.float32)
    kw = dict(num_samples=60, num_steps_per_sample=8, step_size=0.3, burn=30, sampler=ht.Sampler.HMC_NUTS, integrator=ht.Integrator.SPLITTING,
              debug=2, verbose=False, seed=9, desired_accept_rate=0.7)
    th0 = tt(start(128, D, 9, torch.float32), torch.float32)
    a, eps_a = ht.sample(fns, th0, **kw)
    assert "hta_cb_split_kernel" in route(), route()
    os.environ["HAMILTORCH_AMD_JIT"] = "0"
    try:
        b, eps_b = ht.sample(fns, th0, **kw)
        assert "hta_cb_split_kernel" not in route()
    finally:
        del os.environ["HAMILTORCH_AMD_JIT"]
    assert abs(eps_a - eps_b) <= 0.05 * eps_b, (eps_a, eps_b)
    assert 0.01 < eps_a < 3.0 and len(a) == len(b) == 30


class SkipNet(torch.nn.Module):
    """A Linear with a skip connection: not a plain Linear / activation chain, so the native MLP engine does not recognise it."""

    def __init__(self):
        super().__init__()
        self.l1 = torch.nn.Linear(3, 3)
        self.l2 = torch.nn.Linear(3, 1)

    def forward(self, x):
        return self.l2(torch.tanh(self.l1(x)) + x)


def test_sample_split_model_on_an_unrecognised_module(ht, monkeypatch):
    """sample_split_model with a skip-connection module: define_split_model_log_prob's closures carry no `_hta_spec`, the list reaches
    hta_cb_split_kernel and equals the generic route."""
    torch.manual_seed(3)
    net = SkipNet().double()
    N, Ms = 24, 3
    X, Y = torch.randn(N, 3, dtype=torch.float64), torch.randn(N, 1, dtype=torch.float64)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, Y), batch_size=N // Ms, shuffle=False)
    Dn = sum(p.numel() for p in net.parameters())
    th0 = tt(start(96, Dn, 5, torch.float64, scale=0.3), torch.float64)
    kw = dict(model_loss="regression", num_samples=8, num_steps_per_sample=4, step_size=0.02, burn=1, tau_out=4.0, verbose=False, seed=7,
              debug=2)
    a, acc_a = ht.sample_split_model(net, loader, th0, Ms, **kw)
    assert "hta_cb_split_kernel<D=%d,M=3,f64" % Dn in route(), route()
    monkeypatch.setenv("HAMILTORCH_AMD_JIT", "0")
    b, acc_b = ht.sample_split_model(net, loader, th0, Ms, **kw)
    assert "hta_cb_split_kernel" not in route(), route()
    bad = compare(a, [x.cpu().numpy() for x in b], 1e-8, 0.02)
    assert torch.equal(torch.as_tensor(acc_a).cpu()[~bad], torch.as_tensor(acc_b).cpu()[~bad])


def test_fallbacks_keep_their_routes_and_say_why(ht, monkeypatch):
    """native=False, HAMILTORCH_AMD_JIT=0 and a branching subset stay on the torch-evaluated route with the reason in hta_last_route();
    a list of `_hta_spec` closures still runs the native MLP kernel."""
    from hamiltorch_amd import jit
    dtype = torch.float32
    fns = logistic_closures(dtype)
    th0 = tt(start(32, D, 1, dtype), dtype)
    kw = dict(num_samples=5, num_steps_per_sample=3, step_size=0.1, verbose=False, seed=2, integrator=ht.Integrator.SPLITTING)
    want = torch.stack(list(ht.sample(fns, th0, **kw)))
    assert "hta_cb_split_kernel<D=6,M=3,f32,mass=0,kind=symmetric,nodes=" in route(), route()
    out = torch.stack(list(ht.sample(fns, th0, native=False, **kw)))
    assert "hta_cb_split_kernel" not in route() and "not compiled: native=False" in route(), route()
    assert float((out - want).abs().max()) < 2e-4
    monkeypatch.setenv("HAMILTORCH_AMD_JIT", "0")
    ht.sample(fns, th0, **kw)
    assert "hta_cb_split_kernel" not in route() and "not compiled: HAMILTORCH_AMD_JIT=0" in route(), route()
    monkeypatch.delenv("HAMILTORCH_AMD_JIT")

    def branchy(w):
        if w[0] > 0:
            return -(w * w).sum()
        return -0.5 * (w * w).sum() - (w ** 4).sum()

    with pytest.warns(UserWarning, match="not vmap-able"):
        out = ht.sample([fns[0], branchy], th0, **kw)
    assert "not compiled" in route() and "subset 1" in route() and "control flow" in route(), route()
    assert "subset 1" in jit.last_reason() and "control flow" in jit.last_reason()
    assert torch.isfinite(torch.stack(list(out))).all()

    # closures with `_hta_spec` (define_split_model_log_prob on a plain MLP): the native MLP kernel, as before
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Tanh(), torch.nn.Linear(5, 1))
    X = torch.randn(24, 3); Y = torch.randn(24, 1)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, Y), batch_size=8, shuffle=False)
    Dn = sum(p.numel() for p in net.parameters())
    ht.sample_split_model(net, loader, tt(start(20, Dn, 3, dtype, scale=0.3), dtype), 3, model_loss="regression", num_samples=5,
                          num_steps_per_sample=3, step_size=4e-3, tau_out=6.0, verbose=False, seed=11)
    assert "hta_cb_split_kernel" not in route() and "not compiled" not in route() and "mlp" in route(), route()


def test_stale_trace_of_a_list_is_caught_and_retraced(ht):
    """State the closure signatures cannot see (a tensor inside a captured object, edited in place) changes one subset behind a reused
    trace: the check of the kernel's log p against the SUM of the callables catches it, the list is traced again and the results are
    those of the new functions."""
    from hamiltorch_amd import jit

    class Holder:
        pass
    h = Holder()
    h.scale = torch.tensor(1.0, device=dev())
    fns = [lambda w: -0.5 * h.scale * (w ** 4).sum(), lambda w: -0.5 * (w * w).sum()]  # noqa: E731
    th0 = tt(start(64, 3, 8, torch.float32), torch.float32)
    kw = dict(num_samples=12, num_steps_per_sample=6, step_size=0.15, verbose=False, seed=5, integrator=ht.Integrator.SPLITTING)
    a = torch.stack(list(ht.sample(fns, th0, **kw)))
    assert "hta_cb_split_kernel<D=3,M=2" in route(), route()
    traced = jit.stats["traced"]
    a2 = torch.stack(list(ht.sample(fns, th0, **kw)))
    assert jit.stats["traced"] == traced and torch.equal(a, a2)                 # reused, bit-identical
    h.scale.mul_(6.0)                                                           # invisible to the signatures
    b = torch.stack(list(ht.sample(fns, th0, **kw)))
    assert jit.stats["traced"] == traced + 2 and "hta_cb_split_kernel" in route()
    os.environ["HAMILTORCH_AMD_JIT"] = "0"
    try:
        want = torch.stack(list(ht.sample(fns, th0, **kw)))
    finally:
        del os.environ["HAMILTORCH_AMD_JIT"]
    err = (b - want).abs().amax(dim=(0, 2))
    assert float((err > 2e-4).float().mean()) <= 0.03 and not torch.allclose(a, b)
