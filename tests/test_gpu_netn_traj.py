"""GPU parity of the deep-net sampler kernels in TRAJECTORY mode - netn_hmc_kernel<T,PB,WV> (hamiltorch_amd/csrc/netn_hmc.hip), float32
and float64, one, two and four waves per chain, and mlp3_mfma_kernel<ACT> (hamiltorch_amd/csrc/mlp3_mfma.hip) - against
oracle/hmc_oracle.py in float64 on the same Philox draws, through _abi.netn_hmc_sample directly: the mass operands, H_old / H_new /
accept / reject_count, traj_offset and chain_offset are the test's.  Cases, reference and bounds: tests/netn_traj_cases.py; that every
case discriminates: tests/test_netn_traj_cases_cpu.py.

Trajectory 0 has no Metropolis decision before it, so its two energies are held to the oracle's on EVERY chain: H_old pins the draw
indices, the mass factor, the kinetic energy and the full-data log-probability with its (M / prior_scale) log-prior, H_new the stage
loop and the drift on top."""
import functools

import numpy as np
import pytest
import torch

import netn_traj_cases as T

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Out:
    """What one or several launches left: samples[rows, C, D], theta[C, D], rejected[C], h_old / h_new / accept[ntraj, C], routes."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def chains(self, sel):
        return Out(samples=self.samples[:, sel], theta=self.theta[sel], rejected=self.rejected[sel], h_old=self.h_old[:, sel],
                   h_new=self.h_new[:, sel], accept=self.accept[:, sel], theta0=self.theta0[sel], routes=self.routes)


OUTPUTS = ("samples", "theta", "rejected", "h_old", "h_new", "accept")


def operands(case, dtype, chains=None):
    """The case's inputs on the device as the ABI takes them, the mass operands as the product derives them."""
    from hamiltorch_amd import _abi, samplers
    X, Y, th0, im = T.inputs(case.id)
    th0 = th0 if chains is None else th0[chains]
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev())
    theta0 = t(th0)
    kind, imd, mfd = samplers._mass_operands(None if im is None else torch.tensor(im), theta0)      # what the product feeds
    assert kind == (_abi.MASS_NONE if im is None else _abi.MASS_DIAG)
    return t(X), t(Y), theta0, kind, imd, mfd


def launch(case, route, spans=None, chains=None, chain_offset=T.CHAIN_OFFSET):
    """The trajectories of `case` as one launch per (traj_offset, n_traj) span (default: one launch for all) on the rows `chains` of
    the case's chains (default: all), state as sample() keeps it between launches.  Unwritten outputs stay NaN / 255."""
    from hamiltorch_amd import _abi
    dtype = torch.float64 if T.tag(route, case.id) == "f64" else torch.float32
    Xd, Yd, theta0, kind, imd, mfd = operands(case, dtype, chains)
    C, D = theta0.shape
    samples = torch.full((T.n_rows(case), C, D), float("nan"), dtype=dtype, device=dev())
    samples[0] = theta0
    cur = theta0.clone()
    rejected = torch.zeros(C, dtype=torch.int32, device=dev())
    integ = {"symmetric": _abi.SPLIT_SYMMETRIC, "leapfrog": _abi.SPLIT_SYMMETRIC, "rand": _abi.SPLIT_RAND, "kmid": _abi.SPLIT_KMID}[case.integ]
    ho, hn, ac, routes = [], [], [], []
    _abi.set_tuning("netn_waves", T.WAVES.get(route, 1))
    try:
        for n0, cnt in spans or [(0, case.ntraj)]:
            Ho = torch.full((cnt, C), float("nan"), dtype=dtype, device=dev())
            Hn = torch.full_like(Ho, float("nan"))
            acc = torch.full((cnt, C), 255, dtype=torch.uint8, device=dev())
            _abi.netn_hmc_sample(cur, theta0, list(case.dims), case.act, Xd, Yd, case.M, case.Nb, T.taus(case), case.tau_out, float(case.M),
                                 kind, imd, mfd, case.L, case.eps, cnt, n0, T.BURN, case.seed, chain_offset, samples, rejected, Ho, Hn, acc,
                                 integrator=integ, loss=T.LOSS_NAME[case.loss])
            routes.append(_abi.last_route())
            ho.append(Ho); hn.append(Hn); ac.append(acc)
        torch.cuda.synchronize()
    finally:
        _abi.set_tuning("netn_waves", 1)
    n = lambda x: x.cpu().numpy()
    return Out(samples=n(samples), theta=n(cur), rejected=n(rejected), h_old=n(torch.cat(ho)), h_new=n(torch.cat(hn)),
               accept=n(torch.cat(ac)), routes=routes, theta0=n(theta0))


@functools.lru_cache(maxsize=None)
def single(route, cid):
    """One launch for all trajectories of a table case: run once, shared by the tests that compare with it."""
    return launch(T.CASES[cid], route)


def against_oracle(name, tag, got, ref):
    """The assertions of a run against its oracle (tests/netn_traj_cases.py: BOUNDS); prints the figures it asserts on."""
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
    print("%s: oracle acceptance %.2f, %d rejects at burn + 1; %d of %d chains outside the sample band of %g; largest difference inside %.3g; "
          "energies at %.2g of their tolerance" % (name, ref.accept.mean(), (~ref.accept[T.BURN + 1]).sum(), out.sum(), out.size, T.SAMPLE_TOL[tag],
                                                   np.abs(got.samples - ref.samples)[:, inside].max() if inside.any() else np.nan, worst))
    for what, g, w in (("H_old", got.h_old[0], ref.h_old[0]), ("H_new", got.h_new[0], ref.h_new[0])):
        tol = T.ENERGY_TOL[tag] * max(1.0, np.abs(w).max())
        assert np.abs(g - w).max() <= tol, "%s: %s of trajectory 0 differs by %.3g on chain %d (tolerance %.3g)" \
            % (name, what, np.abs(g - w).max(), np.abs(g - w).argmax(), tol)
    assert out.sum() <= T.max_outside(tag, out.size), "%s: %d of %d chains differ, max err %.3g" % (name, out.sum(), out.size, np.abs(got.samples - ref.samples).max())
    # on the chains inside the band: the decisions, their count, and the Q2 reset
    assert np.array_equal(got.accept[:, inside].astype(bool), ref.accept[:, inside])
    assert np.array_equal(got.rejected[inside], ref.rejected[inside])
    reset = inside & ~ref.accept[T.BURN + 1]
    assert reset.sum() >= 2
    assert np.array_equal(got.samples[1][reset], got.theta0[reset])          # the row of burn + 1 IS params_init, to the bit
    assert np.array_equal(got.theta, got.samples[-1])                        # the state handed back is the last row


def same_bits(a, b, what):
    for k in OUTPUTS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("route,cid", T.RUNS, ids=["%s-%s" % r for r in T.RUNS])
def test_trajectories_vs_oracle(route, cid):
    """Every table case on its route: the instance dispatched, the energies of trajectory 0 on every chain, the sample rows chain by
    chain, and on the chains inside the band accept, reject_count and the row of burn + 1."""
    got = single(route, cid)
    assert got.routes == [T.expected_route(route, cid)]
    against_oracle("%s %s %s" % (cid, route, got.routes[0]), T.tag(route, cid), got, T.reference(cid))


@pytest.mark.parametrize("route", ["f32", "f64"])
def test_rows_beyond_the_splits_do_not_leak(route):
    """n10 = n1 with N = M Nb + 5 and the five extra rows of X and Y at 1e6: the full-data log-probability walks M Nb points, not N,
    and a ragged last sweep masks what it reads beyond them - the same bits as n1 in every output."""
    a, b = single(route, "n1"), launch(T.CASES["n10"], route)
    assert b.routes == [T.expected_route(route, "n10")] == a.routes
    same_bits(a, b, "n10 against n1, " + route)
    against_oracle("n10 " + route, route, b, T.reference("n10"))


@pytest.mark.parametrize("route,cid", [("f32", "n1"), ("f64", "n1"), ("mlp3", "w1")], ids=["f32", "f64", "mlp3"])
def test_two_launches_are_one(route, cid):
    """n_traj = 3 then 4 with traj_offset = 0 then 3 (the boundary just after burn + 1, so the second launch starts from a state the
    Q2 reset wrote and recomputes its log-probability): bit-identical to the single launch in the sample rows, the final theta,
    reject_count and every per-trajectory output."""
    one = single(route, cid)
    two = launch(T.CASES[cid], route, spans=[(0, 3), (3, 4)])
    assert two.routes == [T.expected_route(route, cid)] * 2
    same_bits(one, two, "%s %s in two launches" % (cid, route))
    assert one.rejected.sum() > 0 and (one.accept[T.BURN + 1] == 0).sum() >= 2


@pytest.mark.parametrize("route,cid", T.WAVE_RUNS, ids=["%s-%s" % r for r in T.WAVE_RUNS])
def test_wave_variants_vs_oracle(route, cid):
    """Tuning key netn_waves = 2 / 4 (a chain's sweeps over the waves of one workgroup: shared parameter copy and gradient vector,
    likelihood sums exchanged through LDS) on n9 in float32 and n4 in float64: against the oracle like every other route, and the
    energies of trajectory 0 within twice the tolerance of the one-wave run's."""
    tag = T.tag(route, cid)
    got = launch(T.CASES[cid], route)
    assert got.routes == [T.expected_route(route, cid)]
    ref = T.reference(cid)
    against_oracle("%s %s %s" % (cid, route, got.routes[0]), tag, got, ref)
    one = single(tag, cid)
    assert one.routes == [T.expected_route(tag, cid)] and one.routes != got.routes
    for what, g, w in (("H_old", got.h_old[0], one.h_old[0]), ("H_new", got.h_new[0], one.h_new[0])):
        tol = 2 * T.ENERGY_TOL[tag] * max(1.0, np.abs(ref.h_old[0]).max(), np.abs(ref.h_new[0]).max())
        print("%s %s: trajectory 0 %s differs from the one-wave run by %.3g (allowed %.3g)" % (cid, route, what, np.abs(g - w).max(), tol))
        assert np.abs(g.astype(np.float64) - w).max() <= tol


def edge_against_oracle(case, got):
    sel = T.grid_chains(case)
    assert np.isfinite(got.samples).all() and np.isfinite(got.h_old).all() and np.isfinite(got.h_new).all() and (got.accept <= 1).all()
    against_oracle("%s %s" % (case.id, got.routes[0]), "f32", got.chains(sel), T.grid_reference(case.id))


def test_residency_picks_the_smaller_tile():
    """Linear(3, 16)-Tanh-Linear(16, 16)-Tanh-Linear(16, 2), 140 points per split: <float,4,1> takes 83528 bytes of LDS, one workgroup
    per CU, so a launch of C = CUs chains is resident and runs it - and C = CUs + 1 runs <float,2,1> (what the benchmark's 1024 chains
    run on the notebook net).  Both expectations from the launcher's rule restated (tests/netn_traj_cases.py: launcher_rule), both
    runs against the oracle on their first 8 and last 9 chains."""
    n = cus()
    for C, want in ((n, (4, 1)), (n + 1, (2, 1))):
        case = T.res_case(C)
        assert T.resident(case.dims, 4, 1, n) == n and T.launcher_rule(case.dims, case.Nb, C, 1, n) == want
        got = launch(case, "f32")
        assert got.routes == ["netn_hmc_kernel<float,%d,%d>" % want], (C, got.routes)
        edge_against_oracle(case, got)


def test_grid_stride_netn():
    """65537 chains on a grid capped at 65536 workgroups: workgroup 0 runs chain 0, then the last chain in the LDS matrices it has
    just used (the ones / zeros rows of act and dmat, the accumulator blocks, the likelihood slots).  The first 8 and the last 9
    chains against the oracle; the chain beyond the grid bit for bit against a launch of its own (chain_offset moved by the grid),
    where it is a workgroup's first chain."""
    case = T.grid_netn_case()
    got = launch(case, "f32")
    assert got.routes == [T.expected_route("f32", case.id)]
    edge_against_oracle(case, got)
    tail = np.arange(T.GRID_NETN, case.C)
    alone = launch(case, "f32", chains=tail, chain_offset=T.CHAIN_OFFSET + T.GRID_NETN)
    assert alone.routes == got.routes and alone.samples.shape[1] == 1
    same_bits(got.chains(tail), alone, "the chain beyond the grid")


def test_grid_stride_mlp3():
    """2 CUs + 1 chains on mlp3's grid of 2 CUs workgroups: workgroup 0's second chain parks its momentum's W2 share in the slot of
    the workspace its first chain used.  The first 8 and the last 9 chains against the oracle, the chain beyond the grid bit for bit
    against a launch of its own."""
    grid = 2 * cus()
    case = T.grid_mlp3_case(grid + 1)
    got = launch(case, "mlp3")
    assert got.routes == [T.expected_route("mlp3", case.id)] == ["mlp3_mfma_kernel<0>"]
    edge_against_oracle(case, got)
    tail = np.arange(grid, case.C)
    alone = launch(case, "mlp3", chains=tail, chain_offset=T.CHAIN_OFFSET + grid)
    assert alone.routes == got.routes and alone.samples.shape[1] == 1
    same_bits(got.chains(tail), alone, "the chain beyond the grid")


def test_dense_mass_is_refused_before_any_launch():
    """A dense inverse mass on a shape of the small-net kernel: InvalidArguments, and neither the sample rows nor theta are touched."""
    from hamiltorch_amd import _abi, samplers
    case = T.CASES["n1"]
    Xd, Yd, theta0, _, _, _ = operands(case, torch.float32)
    C, D = theta0.shape
    dense = torch.eye(D) * 0.75 + 0.25 / D
    kind, imd, mfd = samplers._mass_operands(dense, theta0)
    assert kind == _abi.MASS_FULL and tuple(imd.shape) == (D, D)
    samples = torch.full((T.n_rows(case), C, D), float("nan"), device=dev())
    cur = theta0.clone()
    rejected = torch.zeros(C, dtype=torch.int32, device=dev())
    with pytest.raises(_abi.InvalidArguments):
        _abi.netn_hmc_sample(cur, theta0, list(case.dims), case.act, Xd, Yd, case.M, case.Nb, T.taus(case), case.tau_out, float(case.M),
                             kind, imd, mfd, case.L, case.eps, case.ntraj, 0, T.BURN, case.seed, T.CHAIN_OFFSET, samples, rejected,
                             loss=T.LOSS_NAME[case.loss])
    torch.cuda.synchronize()
    assert torch.isnan(samples).all() and torch.equal(cur, theta0) and int(rejected.abs().sum()) == 0
