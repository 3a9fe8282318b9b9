"""GPU parity of the compiled leapfrog PATHS (samplers.leapfrog on a (C, D) batch: csrc/jit/path_callback.hip.in): every step's
(theta, p) from identical inputs - nothing is drawn, no Metropolis decision can flip - against the oracle, against the torch-evaluated
route of the same call, and through the fall-back rules.  The route is asserted in every test.
"""
import warnings

import numpy as np
import pytest
import torch

import hmc_oracle as O

pytestmark = pytest.mark.gpu
NP = {torch.float32: np.float32, torch.float64: np.float64}
TAG = {torch.float32: "f32", torch.float64: "f64"}
f32, f64 = torch.float32, torch.float64
D = 6
EPS = 0.1
CHAINS = (2, 64, 65, 200)           # part of a wave; one wave exactly; a tail wave with idle lanes; several waves
STEPS = (1, 2, 7)                   # steps = 1: the first half kick and the half kick taken back meet in one row
HL2P = 0.9189385332046727


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


def rand_spd(d, seed, lo=0.5, hi=1.5):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    P = (Q * np.linspace(lo, hi, d)) @ Q.T
    return 0.5 * (P + P.T)


def masses(d, dtype):
    rng = np.random.default_rng(0)
    return {"none": None, "diag": rng.uniform(0.5, 2.0, d).astype(NP[dtype]), "full": rand_spd(d, 7).astype(NP[dtype])}


def inputs(C, d, dtype, seed=11, scale=1.0):
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((C, d))).astype(NP[dtype]), rng.standard_normal((C, d)).astype(NP[dtype])


def quiet(fn, *a, **kw):
    """A call whose torch-evaluated route may warn (a callable torch.func.vmap cannot batch is evaluated chain by chain)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


# ---- targets: a torch callable for leapfrog() and a numpy gradient, computing in the dtype of its argument, for the oracle -------
_rng = np.random.default_rng(5)
LOG_A = _rng.standard_normal((8, D))
LOG_Y = (_rng.uniform(size=8) > 0.5).astype(np.float64)
LC_P = rand_spd(D, 3)
LC_A = 0.7 * _rng.standard_normal((4, D))


def logistic_fn(dtype, A=LOG_A, y=LOG_Y, prior=0.5):
    """The 6-D Bayesian logistic regression of test_gpu_jit.py::test_other_targets_compiled: closed-over device data."""
    At, yt = tt(A, dtype), tt(y, dtype)

    def fn(w):
        z = At @ w
        return (yt * z - torch.nn.functional.softplus(z)).sum() - prior * (w * w).sum()
    return fn


def logistic_grad(A=LOG_A, y=LOG_Y, prior=0.5):
    def grad(th):
        a, yy = A.astype(th.dtype), y.astype(th.dtype)
        sig = (1.0 / (1.0 + np.exp(-(th @ a.T)))).astype(th.dtype)
        return ((yy - sig) @ a - th.dtype.type(2.0 * prior) * th).astype(th.dtype)
    return grad


def logcosh_fn(dtype):
    """oracle.LogCoshTarget(LC_P, LC_A) in torch."""
    Pt, At = tt(LC_P, dtype), tt(LC_A, dtype)

    def fn(w):
        return -0.5 * (w * (Pt @ w)).sum() - torch.log(torch.cosh(At @ w)).sum()
    return fn


def logcosh_grad():
    """oracle.LogCoshTarget.grad in the dtype of its argument (the oracle's own always computes in float64)."""
    def grad(th):
        P, A = LC_P.astype(th.dtype), LC_A.astype(th.dtype)
        return (-(th @ P) - np.tanh(th @ A.T) @ A).astype(th.dtype)
    return grad


TARGETS = {"logistic": (logistic_fn, logistic_grad), "logcosh": (logcosh_fn, logcosh_grad)}


def funnel_device(w):
    """tests/test_gpu_jit.py: the notebook's funnel written with device-side arithmetic (= oracle.FunnelTarget, s_i = 1)."""
    v, x = w[0], w[1:]
    ll_v = -v * v / 18.0 - 1.0986122886681098 - HL2P
    ll_x = -0.5 * torch.exp(v) * (x * x).sum() + 0.5 * x.numel() * v - x.numel() * HL2P
    return ll_v + ll_x


def band(dtype, wt, wp, d):
    """float64: 1e-9, the project's figure for compiled fp64.  float32: the band of test_gpu_hmc.py::test_leapfrog_batch_vs_oracle."""
    if dtype == f64:
        return dict(rtol=1e-9, atol=1e-9)
    scale = max(1.0, np.abs(np.stack(wt)).max(), np.abs(np.stack(wp)).max())
    return dict(rtol=2e-5, atol=2e-5 * scale * (1 + d / 16))


def check_path(got_t, got_p, wt, wp, tol):
    assert len(got_t) == len(got_p) == len(wt) == len(wp)
    np.testing.assert_allclose(torch.stack(list(got_t)).cpu().numpy(), np.stack(wt), **tol)
    np.testing.assert_allclose(torch.stack(list(got_p)).cpu().numpy(), np.stack(wp), **tol)


def float32_oracle_over_band():
    """Largest |oracle in float32 - oracle in float64| over the float32 band, per target: same inputs, eps = 0.1, 7 steps, 200 chains,
    every mass kind, every row of both paths, no chain exempt."""
    worst = {}
    for name, (_, mk_grad) in TARGETS.items():
        grad = mk_grad()
        th0, p0 = inputs(200, D, f64)
        for kind in ("none", "diag", "full"):
            im = masses(D, f64)[kind]
            wt, wp = O.hmc_leapfrog(th0, p0, grad, 7, EPS, im, return_path=True)
            st, sp = O.hmc_leapfrog(th0.astype(np.float32), p0.astype(np.float32), grad, 7, EPS,
                                    None if im is None else im.astype(np.float32), return_path=True)
            assert np.stack(st).dtype == np.float32 and np.stack(sp).dtype == np.float32
            tol = band(f32, wt, wp, D)
            for a, b in ((st, wt), (sp, wp)):
                a, b = np.stack(a).astype(np.float64), np.stack(b)
                worst[name] = max(worst.get(name, 0.0), float((np.abs(a - b) / (tol["atol"] + tol["rtol"] * np.abs(b))).max()))
    return worst


def test_the_float32_oracle_is_well_inside_the_float32_band():
    """The float32 band (rtol 2e-5, atol 2e-5 * scale * (1 + D / 16)) tests the kernel only if the float32 REFERENCE sits well inside
    it.  Measured on the CPU, oracle in float32 against oracle in float64: the largest difference is 0.0036 of the band for the logistic
    target and 0.0037 for logcosh; the bound asked of a target is a third."""
    worst = float32_oracle_over_band()
    print("float32 oracle / band:", worst)
    assert all(v <= 1.0 / 3.0 for v in worst.values()), worst


@pytest.mark.parametrize("dtype", [f32, f64], ids=["f32", "f64"])
@pytest.mark.parametrize("mass", ["none", "diag", "full"])
@pytest.mark.parametrize("target", ["logistic", "logcosh"])
def test_compiled_path_vs_oracle_every_step(ht, target, mass, dtype):
    """Plain HMC: every row of both paths against oracle.hmc_leapfrog(return_path=True) from identical (theta0, p0); no chain exempt."""
    mk_fn, mk_grad = TARGETS[target]
    fn, grad = mk_fn(dtype), mk_grad()
    im = masses(D, dtype)[mass]
    for C in CHAINS:
        th0, p0 = inputs(C, D, dtype, seed=C)
        for steps in STEPS:
            pt, pp = ht.samplers.leapfrog(tt(th0, dtype), tt(p0, dtype), fn, steps=steps, step_size=EPS, inv_mass=tt(im, dtype),
                                          sampler=ht.Sampler.HMC, integrator=ht.Integrator.EXPLICIT)
            assert route() == "hta_cb_path_kernel<D=6,%s,mass=%s>" % (TAG[dtype], mass), route()
            assert len(pt) == steps and pt[0].shape == (C, D) and pt[0].dtype == dtype
            wt, wp = O.hmc_leapfrog(th0, p0, grad, steps, EPS, im, return_path=True)
            check_path(pt, pp, wt, wp, band(dtype, wt, wp, D))


@pytest.mark.parametrize("mass", ["none", "diag", "full"])
def test_compiled_funnel_path_vs_oracle(ht, mass):
    """The notebook's 11-D funnel, float64 (in float32 its neck amplifies rounding along a path: tests/test_gpu_jit.py)."""
    d = 11
    tgt = O.FunnelTarget(d)
    im = masses(d, f64)[mass]
    for C in (65, 200):
        th0, p0 = inputs(C, d, f64, seed=C, scale=0.5)
        for steps in STEPS:
            pt, pp = ht.samplers.leapfrog(tt(th0, f64), tt(p0, f64), funnel_device, steps=steps, step_size=EPS, inv_mass=tt(im, f64),
                                          sampler=ht.Sampler.HMC, integrator=ht.Integrator.EXPLICIT)
            assert route() == "hta_cb_path_kernel<D=11,f64,mass=%s>" % mass, route()
            wt, wp = O.hmc_leapfrog(th0, p0, tgt.grad, steps, EPS, im, return_path=True)
            check_path(pt, pp, wt, wp, band(f64, wt, wp, d))


def test_compiled_path_equals_the_torch_evaluated_route(ht, monkeypatch):
    """Plain HMC, the same call compiled and with HAMILTORCH_AMD_JIT=0 (vmap(grad_and_value) + the pieces kernels): every step, 1e-9."""
    fn = logistic_fn(f64)
    th0, p0 = (tt(a, f64) for a in inputs(65, D, f64))
    for mass in ("none", "full"):
        kw = dict(step_size=EPS, inv_mass=tt(masses(D, f64)[mass], f64), sampler=ht.Sampler.HMC, integrator=ht.Integrator.EXPLICIT)
        for steps in (1, 3):
            monkeypatch.delenv("HAMILTORCH_AMD_JIT", raising=False)
            a = ht.samplers.leapfrog(th0, p0, fn, steps=steps, **kw)
            assert "hta_cb_path_kernel<D=6,f64" in route(), route()
            monkeypatch.setenv("HAMILTORCH_AMD_JIT", "0")
            b = ht.samplers.leapfrog(th0, p0, fn, steps=steps, **kw)
            assert "hta_cb" not in route() and "HAMILTORCH_AMD_JIT=0" in route(), route()
            check_path(a[0], a[1], [x.cpu().numpy() for x in b[0]], [x.cpu().numpy() for x in b[1]], dict(rtol=1e-9, atol=1e-9))


def logistic_subsets(M, dtype, rows=8):
    rng = np.random.default_rng(0)
    X = rng.standard_normal((M * rows, D))
    y = (rng.uniform(size=M * rows) > 0.5).astype(np.float64)
    parts = [(X[m * rows:(m + 1) * rows], y[m * rows:(m + 1) * rows]) for m in range(M)]
    return [logistic_fn(dtype, A, yy, 0.5 / M) for A, yy in parts], [logistic_grad(A, yy, 0.5 / M) for A, yy in parts]


@pytest.mark.parametrize("kind", ["symmetric", "rand", "kmid"])
def test_compiled_split_path_equals_the_torch_evaluated_route(ht, monkeypatch, kind):
    """M = 3 logistic subsets under each split integrator: every step against the torch-evaluated route of the same call (1e-9), the end
    point against oracle.split_leapfrog (for SPLITTING_RAND with the order both routes drew: one per call, from the seeded stream)."""
    from hamiltorch_amd import util
    M, C, seed = 3, 65, 5
    fns, grads = logistic_subsets(M, f64)
    integ = {"symmetric": ht.Integrator.SPLITTING, "rand": ht.Integrator.SPLITTING_RAND, "kmid": ht.Integrator.SPLITTING_KMID}[kind]
    th0, p0 = inputs(C, D, f64)
    for mass in ("none", "diag", "full"):
        im = masses(D, f64)[mass]
        kw = dict(step_size=EPS, inv_mass=tt(im, f64), sampler=ht.Sampler.HMC, integrator=integ)
        for steps in (1, 3):
            monkeypatch.delenv("HAMILTORCH_AMD_JIT", raising=False)
            util.set_random_seed(seed)
            a = ht.samplers.leapfrog(tt(th0, f64), tt(p0, f64), fns, steps=steps, **kw)
            assert route() == "hta_cb_split_path_kernel<D=6,M=3,f64,mass=%s,%s>" % (mass, kind), route()
            assert len(a[0]) == len(a[1]) == steps and a[0][0].shape == (C, D)
            monkeypatch.setenv("HAMILTORCH_AMD_JIT", "0")
            util.set_random_seed(seed)
            b = ht.samplers.leapfrog(tt(th0, f64), tt(p0, f64), fns, steps=steps, **kw)
            assert "hta_cb" not in route() and "HAMILTORCH_AMD_JIT=0" in route(), route()
            check_path(a[0], a[1], [x.cpu().numpy() for x in b[0]], [x.cpu().numpy() for x in b[1]], dict(rtol=1e-9, atol=1e-9))
            util.set_random_seed(seed)
            perm = util.split_permutation(util.next_stream_seed(), 0, M) if kind == "rand" else None
            et, ep = O.split_leapfrog(th0, p0, grads, steps, EPS, im, kind, perm)
            # (the tolerances of test_gpu_mlp.py::test_split_kinds_leapfrog_api_vs_reference_fixture)
            np.testing.assert_allclose(a[0][-1].cpu().numpy(), et, rtol=3e-5, atol=3e-5)
            np.testing.assert_allclose(a[1][-1].cpu().numpy(), ep, rtol=3e-4, atol=3e-4)

def test_one_chain_keeps_the_reference_route(ht, monkeypatch):
    """A (D,) params is ONE chain: never a path kernel, the rows are (D,) tensors and equal, bit for bit, those of the torch-evaluated
    route on the same chain as a batch of one."""
    fn = logistic_fn(f32)
    th0, p0 = (tt(a, f32) for a in inputs(1, D, f32))
    kw = dict(steps=4, step_size=EPS, sampler=ht.Sampler.HMC, integrator=ht.Integrator.EXPLICIT)
    pt, pp = ht.samplers.leapfrog(th0[0], p0[0], fn, **kw)
    assert "hta_cb" not in route() and "one chain" in route(), route()
    assert len(pt) == len(pp) == 4 and all(t.shape == (D,) for t in pt) and all(t.shape == (D,) for t in pp)
    monkeypatch.setenv("HAMILTORCH_AMD_JIT", "0")
    bt, bp = ht.samplers.leapfrog(th0, p0, fn, **kw)
    assert all(torch.equal(a, b[0]) for a, b in zip(pt, bt)) and all(torch.equal(a, b[0]) for a, b in zip(pp, bp))
    monkeypatch.delenv("HAMILTORCH_AMD_JIT")
    fns, _ = logistic_subsets(3, f32)
    st, sp = ht.samplers.leapfrog(th0[0], p0[0], fns, **dict(kw, integrator=ht.Integrator.SPLITTING))
    assert "hta_cb" not in route() and "one chain" in route(), route()
    assert len(st) == 4 and st[0].shape == (D,) and sp[0].shape == (D,)
    ct, cp = ht.samplers.leapfrog(th0, p0, fns, **dict(kw, integrator=ht.Integrator.SPLITTING))       # as a batch of one: compiled
    assert "hta_cb_split_path_kernel<D=6,M=3,f32" in route(), route()
    np.testing.assert_allclose(torch.stack(st).cpu().numpy(), torch.stack(ct)[:, 0].cpu().numpy(), rtol=2e-5, atol=2e-5)


def test_fallbacks_keep_the_torch_evaluated_route_and_say_why(ht, monkeypatch):
    """Data-dependent control flow, D = 65, pass_grad and HAMILTORCH_AMD_JIT=0: the torch-evaluated route, its reason in hta_last_route(),
    its results (equal to those of the same call with the compiler switched off)."""
    def branchy(w):
        if w[0] > 0:
            return -(w * w).sum()
        return -0.5 * (w * w).sum() - (w ** 4).sum()

    quartic = lambda w: -(w ** 4).sum() - 0.5 * (w * w).sum()  # noqa: E731
    wide = lambda w: -0.5 * (w * w).sum() - 0.1 * (w ** 4).sum()  # noqa: E731
    kw = dict(steps=3, step_size=EPS, sampler=ht.Sampler.HMC, integrator=ht.Integrator.EXPLICIT)
    cases = [("control flow", branchy, 4, {}), ("D = 65", wide, 65, {}),
             ("pass_grad supplies the gradient", quartic, 4, dict(pass_grad=lambda w: -4 * w ** 3 - w))]
    for reason, fn, d, extra in cases:
        th0, p0 = (tt(a, f32) for a in inputs(32, d, f32, scale=0.5))
        monkeypatch.delenv("HAMILTORCH_AMD_JIT", raising=False)
        a = quiet(ht.samplers.leapfrog, th0, p0, fn, **kw, **extra)
        assert "not compiled" in route() and reason in route() and "hta_cb" not in route(), route()
        monkeypatch.setenv("HAMILTORCH_AMD_JIT", "0")
        b = quiet(ht.samplers.leapfrog, th0, p0, fn, **kw, **extra)
        for x, y in zip(a[0] + a[1], b[0] + b[1]):
            assert torch.isfinite(x).all() and torch.equal(x, y)
    # the switch itself, and the compiled route of the same callable next to it
    th0, p0 = (tt(a, f32) for a in inputs(32, 4, f32, scale=0.5))
    b = ht.samplers.leapfrog(th0, p0, quartic, **kw)
    assert "not compiled" in route() and "HAMILTORCH_AMD_JIT=0" in route(), route()
    monkeypatch.delenv("HAMILTORCH_AMD_JIT")
    a = ht.samplers.leapfrog(th0, p0, quartic, **kw)
    assert route() == "hta_cb_path_kernel<D=4,f32,mass=none>", route()
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert torch.isfinite(y).all()
        np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), rtol=2e-5, atol=2e-5)
    # a list with an unsupported member: refused as a whole, the reason names the member
    fns, _ = logistic_subsets(2, f32)
    th0, p0 = (tt(a, f32) for a in inputs(8, D, f32, scale=0.5))
    out = quiet(ht.samplers.leapfrog, th0, p0, fns + [branchy], **dict(kw, integrator=ht.Integrator.SPLITTING))
    assert "not compiled" in route() and "subset 2" in route(), route()
    assert torch.isfinite(torch.stack(out[0])).all()


def test_stale_trace_is_caught_by_the_check_against_the_callable(ht, monkeypatch):
    """tests/test_gpu_jit.py's rule for sample(), here for leapfrog(): a tensor inside a captured object edited in place is invisible to
    the trace's signature; the check of the end points against the callable catches it, the callable is traced again, and the path is
    the NEW function's."""
    from hamiltorch_amd import jit

    class Holder:
        pass
    h = Holder()
    h.scale = torch.tensor(1.0, device=dev())
    fn = lambda w: -0.5 * h.scale * (w ** 4).sum() - 0.5 * (w * w).sum()  # noqa: E731
    th0, p0 = (tt(a, f32) for a in inputs(64, 3, f32, scale=0.7))
    kw = dict(steps=5, step_size=0.15, sampler=ht.Sampler.HMC, integrator=ht.Integrator.EXPLICIT)
    a = torch.stack(ht.samplers.leapfrog(th0, p0, fn, **kw)[0])
    traced = jit.stats["traced"]
    a2 = torch.stack(ht.samplers.leapfrog(th0, p0, fn, **kw)[0])
    assert jit.stats["traced"] == traced and torch.equal(a, a2)                 # reused, bit-identical
    h.scale.mul_(6.0)                                                           # invisible to the signature
    b = torch.stack(ht.samplers.leapfrog(th0, p0, fn, **kw)[0])
    assert jit.stats["traced"] == traced + 1 and route() == "hta_cb_path_kernel<D=3,f32,mass=none>", route()
    monkeypatch.setenv("HAMILTORCH_AMD_JIT", "0")
    want = torch.stack(ht.samplers.leapfrog(th0, p0, fn, **kw)[0])
    np.testing.assert_allclose(b.cpu().numpy(), want.cpu().numpy(), rtol=2e-5, atol=2e-5 * float(want.abs().max()))
    assert not torch.allclose(a, b)


def test_a_divergent_chain_keeps_its_non_finite_rows_to_itself(ht):
    """eps = 40 on log p = -w_0^4 - |w_1:|^2 / 2.  A chain with w_0 = p_0 = 0 keeps that coordinate at zero exactly and its other
    coordinates on a linear (unstable, finite) recursion; ONE chain starts at w_0 = 1, where the quartic term cubes the state at every
    step until it overflows.  Its rows become non-finite, every other chain matches the oracle, nothing is raised."""
    d, C, steps, bad = 4, 70, 8, 37
    fn = lambda w: -(w[0] ** 4) - 0.5 * (w[1:] * w[1:]).sum()  # noqa: E731

    def grad(th):
        g = -th.copy()
        g[..., 0] = -4.0 * th[..., 0] ** 3
        return g

    th0, p0 = inputs(C, d, f64, scale=0.5)
    th0[:, 0] = 0.0; p0[:, 0] = 0.0
    th0[bad, 0] = 1.0
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        pt, pp = ht.samplers.leapfrog(tt(th0, f64), tt(p0, f64), fn, steps=steps, step_size=40.0, sampler=ht.Sampler.HMC,
                                      integrator=ht.Integrator.EXPLICIT)
    assert route() == "hta_cb_path_kernel<D=4,f64,mass=none>", route()
    assert not [w for w in caught if "disagrees" in str(w.message)]             # the end-point check exempts what is non-finite on both sides
    got_t, got_p = torch.stack(pt).cpu().numpy(), torch.stack(pp).cpu().numpy()
    assert np.isfinite(got_t[0, bad]).all() and np.isfinite(got_p[0, bad]).all()
    assert not np.isfinite(got_t[-1, bad, 0]) and not np.isfinite(got_p[-1, bad, 0])        # (the other coordinates do not see w_0)
    with np.errstate(all="ignore"):
        wt, wp = O.hmc_leapfrog(th0, p0, grad, steps, 40.0, None, return_path=True)
    ok = np.arange(C) != bad
    for got, want in ((got_t, np.stack(wt)), (got_p, np.stack(wp))):
        assert np.isfinite(got[:, ok]).all()
        for n in range(steps):                                                  # (the rows grow by ~1600 x per step: relative to each row's size)
            np.testing.assert_allclose(got[n, ok], want[n, ok], rtol=1e-9, atol=1e-9 * np.abs(want[n, ok]).max())
