"""GPU parity of the one-hidden-layer MLP sampler kernels in TRAJECTORY mode - mlp_mfma_kernel (csrc/mlp_mfma_dev.hpp) and
mlp1_hmc_kernel (csrc/mlp_hmc.hip), float32 and float64 - against oracle/hmc_oracle.py in float64 on the same Philox draws, through
_abi.mlp_hmc_sample directly: the route, the mass operands, H_old / H_new / accept / reject_count, traj_offset and chain_offset are
the test's.  Cases, reference and bounds: tests/mlp_traj_cases.py; that every case discriminates: tests/test_mlp_traj_cases_cpu.py.

Trajectory 0 has no Metropolis decision before it, so its two energies are held to the oracle's on EVERY chain: H_old pins the draw
indices, the mass factor, the kinetic energy and the full-data log-probability, H_new the stage loop and the drift on top."""
import functools

import numpy as np
import pytest
import torch

import mlp_traj_cases as T

pytestmark = pytest.mark.gpu

DTYPE = {"mfma": torch.float32, "valu": torch.float32, "f64": torch.float64}
TAG = {"mfma": "f32", "valu": "f32", "f64": "f64"}


def dev():
    return torch.device("cuda:0")


class Out:
    """What one or several launches left: samples[rows, C, D], theta[C, D], rejected[C], h_old / h_new / accept[ntraj, C], routes."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def launch(case, route, spans=None, chains=None, chain_offset=T.CHAIN_OFFSET):
    """The trajectories of `case` as one launch per (traj_offset, n_traj) span (default: one launch for all) on the rows `chains` of
    the case's chains (default: all), state as sample() keeps it between launches.  Unwritten outputs stay NaN / 255."""
    from hamiltorch_amd import _abi, samplers
    dtype = DTYPE[route]
    X, Y, th0, im = T.inputs(case.id)
    th0 = th0 if chains is None else th0[chains]
    C, D = th0.shape
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev())
    Xd, Yd, theta0 = t(X), t(Y), t(th0)
    kind, imd, mfd = samplers._mass_operands(None if im is None else torch.tensor(im), theta0)      # what the product feeds
    assert kind == (_abi.MASS_NONE if im is None else _abi.MASS_DIAG)
    samples = torch.full((T.n_rows(case), C, D), float("nan"), dtype=dtype, device=dev())
    samples[0] = theta0
    cur = theta0.clone()
    rejected = torch.zeros(C, dtype=torch.int32, device=dev())
    integ = {"symmetric": _abi.SPLIT_SYMMETRIC, "leapfrog": _abi.SPLIT_SYMMETRIC, "rand": _abi.SPLIT_RAND, "kmid": _abi.SPLIT_KMID}[case.integ]
    ho, hn, ac, routes = [], [], [], []
    _abi.set_tuning("mlp_valu", 1 if route == "valu" else 0)
    try:
        for n0, cnt in spans or [(0, case.ntraj)]:
            Ho = torch.full((cnt, C), float("nan"), dtype=dtype, device=dev())
            Hn = torch.full_like(Ho, float("nan"))
            acc = torch.full((cnt, C), 255, dtype=torch.uint8, device=dev())
            _abi.mlp_hmc_sample(cur, theta0, case.n_in, case.H, case.act, Xd, Yd, case.M, case.Nb, list(T.TAU), case.tau_out, float(case.M),
                                kind, imd, mfd, case.L, case.eps, cnt, n0, T.BURN, case.seed, chain_offset, samples, rejected, Ho, Hn, acc,
                                integrator=integ)
            routes.append(_abi.last_route())
            ho.append(Ho); hn.append(Hn); ac.append(acc)
        torch.cuda.synchronize()
    finally:
        _abi.set_tuning("mlp_valu", 0)
    n = lambda x: x.cpu().numpy()
    return Out(samples=n(samples), theta=n(cur), rejected=n(rejected), h_old=n(torch.cat(ho)), h_new=n(torch.cat(hn)),
               accept=n(torch.cat(ac)), routes=routes, theta0=n(theta0))


@functools.lru_cache(maxsize=None)
def single(route, cid):
    """One launch for all trajectories of a table case: run once, shared by the tests that compare with it."""
    return launch(T.CASES[cid], route)


def against_oracle(name, tag, got, ref):
    """The assertions of a run against its oracle (tests/mlp_traj_cases.py: BOUNDS); prints the figures it asserts on."""
    for a in (got.samples, got.theta, got.h_old, got.h_new):
        assert np.isfinite(a).all(), "%s: an output was not written (or is not finite)" % name
    assert set(np.unique(got.accept)) <= {0, 1}
    # trajectory 0: every chain, no exemption
    worst = 0.0
    for what, g, w in (("H_old", got.h_old[0], ref.h_old[0]), ("H_new", got.h_new[0], ref.h_new[0])):
        tol = T.ENERGY_TOL[tag] * max(1.0, np.abs(w).max())
        err = np.abs(g - w).max()
        worst = max(worst, err / tol)
        print("%s: trajectory 0 %s off by %.3g, tolerance %.3g (%.2g of it)" % (name, what, err, tol, err / tol))
    # sample rows chain by chain
    out = T.outside(got.samples.astype(np.float64), ref.samples, T.SAMPLE_TOL[tag])
    inside = ~out
    print("%s: %d of %d chains outside the sample band of %g; largest difference inside %.3g; energies at %.2g of their tolerance"
          % (name, out.sum(), out.size, T.SAMPLE_TOL[tag], np.abs(got.samples - ref.samples)[:, inside].max(), worst))
    for what, g, w in (("H_old", got.h_old[0], ref.h_old[0]), ("H_new", got.h_new[0], ref.h_new[0])):
        tol = T.ENERGY_TOL[tag] * max(1.0, np.abs(w).max())
        assert np.abs(g - w).max() <= tol, "%s: %s of trajectory 0 differs by %.3g on chain %d (tolerance %.3g)" \
            % (name, what, np.abs(g - w).max(), np.abs(g - w).argmax(), tol)
    assert out.mean() <= T.MAX_OUTSIDE[tag], "%s: %d of %d chains differ, max err %.3g" % (name, out.sum(), out.size, np.abs(got.samples - ref.samples).max())
    # on the chains inside the band: the decisions, their count, and the Q2 reset
    assert np.array_equal(got.accept[:, inside].astype(bool), ref.accept[:, inside])
    assert np.array_equal(got.rejected[inside], ref.rejected[inside])
    reset = inside & ~ref.accept[T.BURN + 1]
    assert reset.sum() >= 2
    assert np.array_equal(got.samples[1][reset], got.theta0[reset])          # the row of burn + 1 IS params_init, to the bit
    assert np.array_equal(got.theta, got.samples[-1])                        # the state handed back is the last row


@pytest.mark.parametrize("route,cid", T.RUNS, ids=["%s-%s" % r for r in T.RUNS])
def test_trajectories_vs_oracle(route, cid):
    """Every table case on its route: the instance dispatched, the energies of trajectory 0 on every chain, the sample rows chain by
    chain, and on the chains inside the band accept, reject_count and the row of burn + 1."""
    got = single(route, cid)
    assert got.routes == [T.expected_route(route, cid)]
    against_oracle("%s %s %s" % (cid, route, got.routes[0]), TAG[route], got, T.reference(cid))


@pytest.mark.parametrize("route", ["mfma", "valu"])
def test_rows_beyond_the_splits_do_not_leak(route):
    """m9 = m1 with N = M Nb + 5 and the five extra rows of X and Y at 1e6: the full-data log-probability walks M Nb points, not N,
    and a padded last chunk masks what it reads beyond them - the same bits as m1 in every output."""
    a, b = single(route, "m1"), launch(T.CASES["m9"], route)
    assert b.routes == [T.expected_route(route, "m9")] == a.routes
    for k in ("samples", "theta", "rejected", "h_old", "h_new", "accept"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    against_oracle("m9 " + route, "f32", b, T.reference("m9"))


@pytest.mark.parametrize("route", ["mfma", "valu", "f64"])
def test_two_launches_are_one(route):
    """m1 as n_traj = 3 then 4 with traj_offset = 0 then 3 (the boundary just after burn + 1, so the second launch starts from a
    state the Q2 reset wrote and recomputes its log-probability): bit-identical to the single launch in the sample rows, the final
    theta, reject_count and every per-trajectory output."""
    one = single(route, "m1")
    two = launch(T.CASES["m1"], route, spans=[(0, 3), (3, 4)])
    assert two.routes == [T.expected_route(route, "m1")] * 2
    for k in ("samples", "theta", "rejected", "h_old", "h_new", "accept"):
        assert np.array_equal(getattr(one, k), getattr(two, k)), k
    assert one.rejected.sum() > 0 and (one.accept[T.BURN + 1] == 0).sum() >= 2


@pytest.mark.parametrize("kind", ["mfma", "valu"])
def test_grid_stride_over_chains(kind):
    """One chain more than the launch has workgroups (8192 / 4096): workgroup 0 runs chain 0, then the last chain in the LDS
    buffers it has just used.  The first 8 and the last 9 chains against the oracle; the chains beyond the grid bit for bit against
    a launch of their own (chain_offset moved by the grid), where they are a workgroup's first chain."""
    case, ref = T.GRID_CASES[kind], T.grid_reference(kind)
    grid = T.GRID[kind]
    got = launch(case, kind)
    assert got.routes == [T.expected_route(kind, case.id)]
    assert np.isfinite(got.samples).all() and np.isfinite(got.h_old).all() and (got.accept <= 1).all()
    sel = T.grid_chains(case)
    part = Out(samples=got.samples[:, sel], theta=got.theta[sel], rejected=got.rejected[sel], h_old=got.h_old[:, sel],
               h_new=got.h_new[:, sel], accept=got.accept[:, sel], theta0=got.theta0[sel])
    against_oracle("%s %s" % (case.id, got.routes[0]), "f32", part, ref)
    tail = np.arange(grid, case.C)
    alone = launch(case, kind, chains=tail, chain_offset=T.CHAIN_OFFSET + grid)
    assert alone.routes == got.routes and alone.samples.shape[1] == case.C - grid
    for k in ("samples", "h_old", "h_new", "accept"):
        assert np.array_equal(getattr(got, k)[:, tail], getattr(alone, k)), k
    assert np.array_equal(got.theta[tail], alone.theta) and np.array_equal(got.rejected[tail], alone.rejected)


# ---- through the Python API: the engine hands inv_mass / mass_factor to the kernel once the values are not all ones ----------------------
def _api_setup(kind):
    case = T.API_CASES[kind]
    X, Y, th0, im = T.inputs(case.id)
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(case.n_in, case.H), torch.nn.Tanh(), torch.nn.Linear(case.H, 1)).to(dev())
    kw = dict(model_loss="regression", num_samples=case.ntraj, num_steps_per_sample=case.L, step_size=case.eps, burn=T.BURN,
              inv_mass=torch.tensor(im, device=dev()), tau_out=case.tau_out, tau_list=torch.tensor(T.TAU), verbose=False, seed=case.seed)
    return case, net, torch.tensor(X), torch.tensor(Y).reshape(-1, 1), torch.tensor(th0, device=dev()), kw


def _api_cmp(name, out, ref):
    got = np.stack([o.cpu().numpy() for o in out]).astype(np.float64)
    assert np.isfinite(got).all()
    bad = T.outside(got, ref.samples, T.SAMPLE_TOL["f32"])
    print("%s: %d of %d chains outside the sample band" % (name, bad.sum(), bad.size))
    assert bad.mean() <= T.MAX_OUTSIDE["f32"], "%s: %d of %d chains differ, max err %.3g" % (name, bad.sum(), bad.size, np.abs(got - ref.samples).max())


def test_sample_split_model_with_a_diagonal_mass():
    import hamiltorch_amd as ht
    from hamiltorch_amd import _abi, bnn, mlp
    case, net, X, Y, th0, kw = _api_setup("split")
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, Y), batch_size=case.Nb, shuffle=False)
    ref = T.api_reference("split")
    out = ht.sample_split_model(net, loader, th0, case.M, **kw)
    route = _abi.last_route()
    assert route.startswith(("mlp_mfma_kernel<", "mlp1_hmc_kernel<")), route
    _api_cmp("sample_split_model " + route, out, ref)
    _api_cmp("sample_split_model native=False", ht.sample_split_model(net, loader, th0, case.M, native=False, **kw), ref)
    sizes = [w.nelement() for w in net.parameters()]; shapes = [w.shape for w in net.parameters()]
    fl = bnn.define_split_model_log_prob(net, "regression", loader, case.M, sizes, shapes, kw["tau_list"], case.tau_out, device=dev(), verbose=False)
    assert mlp.split_engine(fl, th0) is not None


def test_sample_model_with_a_diagonal_mass():
    import hamiltorch_amd as ht
    from hamiltorch_amd import _abi, bnn, mlp
    case, net, X, Y, th0, kw = _api_setup("full")
    ref = T.api_reference("full")
    out = ht.sample_model(net, X, Y, th0, **kw)
    route = _abi.last_route()
    assert route.startswith(("mlp_mfma_kernel<", "mlp1_hmc_kernel<")), route
    _api_cmp("sample_model " + route, out, ref)
    _api_cmp("sample_model native=False", ht.sample_model(net, X, Y, th0, native=False, **kw), ref)
    sizes = [w.nelement() for w in net.parameters()]; shapes = [w.shape for w in net.parameters()]
    f = bnn.define_model_log_prob(net, "regression", X, Y, sizes, shapes, kw["tau_list"], case.tau_out, device=dev())
    assert mlp.hmc_engine(f, th0) is not None
