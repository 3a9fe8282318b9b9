"""GPU parity of the plain-HMC kernels for Gaussian targets in TRAJECTORY mode - hmc_gauss_small_kernel<T,D,MASS,WS,DIAG>,
hmc_gauss_eig_kernel<T,D,DIAG>, hmc_gauss_quad_kernel<D,DIAG,LB[,VAR]>, the one-launch quad route, hmc_gauss_wave_kernel<T,R,MASS> and
hmc_gauss_wave_eig_kernel<T,R> (hamiltorch_amd/csrc/hmc_gaussian.hip) - against oracle/hmc_oracle.py:sample_hmc in float64 on the same
Philox draws, through _abi.hmc_gaussian_sample directly: cur, theta_init, the workspace, samples, reject_count, H_old / H_new / accept,
traj_offset and chain_offset are the test's.  Cases, reference, bounds and the launcher's rules restated: tests/gauss_traj_cases.py;
that every case discriminates (its step size makes the oracle reject): tests/test_gauss_traj_cases_cpu.py.

Every launch asserts _abi.last_route() against the restated rule, so no run compares a kernel with itself or lands on another one
silently.  Trajectory 0 has no Metropolis decision before it, so its two energies are held to the oracle's on EVERY chain: H_old pins
the draw indices, the momentum law with its mass factor, the kinetic term and log p with its mean and log_norm, H_new the whole step
loop on top.  The rows, `cur`, accept, reject_count and the Q2 reset row pin the bookkeeping every kernel restates.  Outputs start as
NaN / 255 / -7 and the workspace as 0xFF bytes, so an element nobody wrote - or a record read that was never drawn - shows."""
import functools

import numpy as np
import pytest
import torch

import gauss_traj_cases as T

pytestmark = pytest.mark.gpu
OUTPUTS = ("rows", "cur", "rejected", "h_old", "h_new", "accept")


def dev():
    return torch.device("cuda:0")


class Out:
    """What one or several launches left: rows[T - burn, C, D], cur[C, D], rejected[C], h_old / h_new / accept[T, C] (None on a route
    without them), routes."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def chains(self, sel):
        pick = lambda a: None if a is None else a[:, sel]
        return Out(rows=self.rows[:, sel], cur=self.cur[sel], rejected=self.rejected[sel], h_old=pick(self.h_old), h_new=pick(self.h_new),
                   accept=pick(self.accept), theta0=self.theta0[sel], routes=self.routes)


def launch(case, route, spans=None, pad=0):
    """The trajectories of `case` on `route`, one launch per (traj_offset, n_traj) span (default: one launch for all), the state
    travelling through `cur`.  pad: that many rows of 1e6 behind the last chain in cur and theta_init (and untouched entries behind
    reject_count), C unchanged.  Every launch is held to the restated launcher; a guard row in front of and behind the sample rows,
    the sentinel in row 0, the pad rows and the entries behind reject_count must come back as they went in."""
    from hamiltorch_amd import _abi
    r = T.ROUTES[route]
    dtype, npdt = (torch.float64, np.float64) if r.f64 else (torch.float32, np.float32)
    P, mu = T.inputs_of(case.D)
    C, D, n_rows = case.C, case.D, case.ntraj - case.burn
    t = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev())
    Pd, mud = t(P), t(mu)
    kind, im, mf = T.mass_operands(case, npdt)
    imd, mfd = t(im), t(mf)
    init_all = torch.full((C + pad, D), 1e6, dtype=dtype, device=dev())
    init_all[:C] = t(T.starts(case))
    cur_all = init_all.clone()
    theta0, cur = init_all[:C], cur_all[:C]
    rows_all = torch.full((n_rows + 2, C, D), float("nan"), dtype=dtype, device=dev())
    rows = rows_all[1:-1]
    rows[0] = theta0 + 1.0          # (a sentinel: no kernel writes row 0 - or reads it; hta_run_begin fills it in a run of sample())
    rej_all = torch.full((C + pad,), -7, dtype=torch.int32, device=dev())
    rej_all[:C] = 0
    ws = None
    if r.ws != "no":
        nbytes = _abi.gaussian_workspace_bytes(C, D, case.ntraj, Pd.element_size())
        assert nbytes == T.workspace_bytes(C, D, case.ntraj, Pd.element_size())
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev())
    ho, hn, ac, routes = [], [], [], []
    try:
        for k, v in r.keys.items():
            _abi.set_tuning(k, v)
        for k, v in dict(T.DEFAULT_KEYS, **r.keys).items():
            assert _abi.get_tuning(k) == v, (k, v, _abi.get_tuning(k))
        if r.ws == "prepared":
            _abi.hmc_gaussian_prepare(cur, Pd, kind, mfd, C, D, case.ntraj, ws)
        for n0, cnt in spans or [(0, case.ntraj)]:
            Ho = Hn = acc = None
            if r.diag:
                Ho = torch.full((cnt, C), float("nan"), dtype=dtype, device=dev())
                Hn = torch.full_like(Ho, float("nan"))
                acc = torch.full((cnt, C), 255, dtype=torch.uint8, device=dev())
            _abi.hmc_gaussian_sample(cur, theta0, Pd, mud, T.log_norm(D), kind, imd, mfd, case.L, T.eps_of(case), cnt, n0, case.burn, case.seed,
                                     T.CHAIN_OFFSET, rows, rej_all[:C], H_old=Ho, H_new=Hn, accept=acc, workspace=ws)
            routes.append(_abi.last_route())
            assert routes[-1] == T.expected_route(case, route, cnt), (case.id, route, cnt, routes[-1], T.expected_route(case, route, cnt))
            ho.append(Ho); hn.append(Hn); ac.append(acc)
        torch.cuda.synchronize()
    finally:
        _abi.reset_tuning()
        if r.ws == "prepared":
            _abi.hmc_gaussian_forget(ws)
    assert bool(torch.isnan(rows_all[0]).all()) and bool(torch.isnan(rows_all[-1]).all()), "a row outside the sample rows was written"
    assert torch.equal(rows[0], theta0 + 1.0), "row 0 was written"
    rows[0] = theta0
    if pad:
        assert bool((init_all[C:] == 1e6).all()) and bool((cur_all[C:] == 1e6).all()) and bool((rej_all[C:] == -7).all())
    n = lambda x: x.cpu().numpy()
    cat = lambda xs: n(torch.cat(xs)) if r.diag else None
    return Out(rows=n(rows), cur=n(cur), rejected=n(rej_all[:C]), h_old=cat(ho), h_new=cat(hn), accept=cat(ac), routes=routes, theta0=n(theta0))


@functools.lru_cache(maxsize=None)
def single(cid, route):
    """One launch for all trajectories of a table case on a route: run once, shared by the tests that compare with it."""
    return launch(T.CASES[cid], route)


def energy_shares(route, case, got, ref):
    """H_old and H_new of trajectory 0 on every chain as shares of their tolerance: {name: (largest share, its chain, its error)}."""
    share = {}
    if T.ROUTES[route].diag:
        for what, g, w in (("H_old", got.h_old[0], ref.h_old[0]), ("H_new", got.h_new[0], ref.h_new[0])):
            s = np.abs(g - w) / T.h_tol(T.tag(route), case, w)
            share[what] = (s.max(), int(s.argmax()), np.abs(g - w).max())
    return share


def against_oracle(name, route, case, got, ref):
    """The assertions of a run against its oracle on rows, cur and the decisions (tests/gauss_traj_cases.py: BOUNDS); prints the figures
    it asserts on and, for the table, the energy shares test_energies_of_trajectory_0_vs_oracle asserts on."""
    tag, kernel = T.tag(route), got.routes[0]
    diag = T.ROUTES[route].diag
    for a in (got.rows, got.cur) + ((got.h_old, got.h_new) if diag else ()):
        assert np.isfinite(a).all(), "%s: an output was not written (or is not finite)" % name
    n_c = got.cur.shape[0]
    if diag:
        assert set(np.unique(got.accept)) <= {0, 1}
    share = energy_shares(route, case, got, ref)
    band = T.row_band(tag, kernel, case.D, ref.rows)
    out = T.outside(got.rows.astype(np.float64), got.cur.astype(np.float64), ref, band)
    inside = ~out
    err_in = max(np.abs(got.rows - ref.rows)[:, inside].max(), np.abs(got.cur - ref.cur)[inside].max()) if inside.any() else np.nan
    b1 = case.burn + 1
    print("%-8s %-16s %-46s oracle acceptance %.2f / %s rejects at burn + 1 of %d; trajectory 0 H_old %s, H_new %s of their tolerance; rows %.2g of the band %.3g, %d outside"
          % (case.id, route, kernel, ref.accept.mean(), (~ref.accept[b1]).sum() if 0 <= b1 < case.ntraj else "-", n_c,
             "%.2g" % share["H_old"][0] if share else "-", "%.2g" % share["H_new"][0] if share else "-", err_in / band, band, out.sum()))
    assert out.sum() <= T.max_outside(tag, n_c), "%s: %d of %d chains outside the band, max err %.3g" % (name, out.sum(), n_c, np.nanmax(np.abs(got.rows - ref.rows)))
    # on the chains inside the band: the decisions, their count, the acceptance rate, the Q2 reset, the state handed back
    if diag:
        assert np.array_equal(got.accept[:, inside].astype(bool), ref.accept[:, inside]), "%s: accept differs" % name
    assert np.array_equal(got.rejected[inside], ref.rejected[inside]), "%s: reject_count differs" % name
    assert np.array_equal(1.0 - got.rejected[inside] / float(case.ntraj), ref.acc_rate[inside])
    if 0 <= b1 < case.ntraj:
        reset = inside & ~ref.accept[b1]
        assert np.array_equal(got.rows[1][reset], got.theta0[reset]), "%s: the row of burn + 1 of a rejecting chain is not theta_init" % name
    if case.ntraj - 1 > case.burn:
        assert np.array_equal(got.cur, got.rows[-1]), "%s: the state handed back is not the last row" % name


def same_bits(a, b, what):
    for k in OUTPUTS:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), "%s: %s differs" % (what, k)


def same_values(a, b, tag, band, what, case=None, n0=None):
    """Two runs of the same draws whose arithmetic differs: chain by chain the same decisions and reject_count, rows and cur within
    `band`; the chains of which that does not hold are counted and may be as many as the band exempts.  case, n0: the two runs are a
    run and the same run cut in two at trajectory n0 - then H_old and H_new of EVERY trajectory of the other chains agree: up to and
    including trajectory n0 (the same float32 start point on both sides) within the tolerance of a trajectory-0 energy, beyond it
    within the untightened one (tests/gauss_traj_cases.py: TWO LAUNCHES)."""
    with np.errstate(invalid="ignore"):
        far = ~((np.abs(a.rows - b.rows).max(axis=(0, 2)) <= band) & (np.abs(a.cur - b.cur).max(axis=1) <= band))
    flipped = a.rejected != b.rejected
    if a.accept is not None and b.accept is not None:
        flipped |= (a.accept != b.accept).any(axis=0)
    bad = far | flipped
    err = np.abs(a.rows - b.rows)[:, ~bad].max() if (~bad).any() else np.nan
    print("%s: %d of %d chains differ (%d by a decision); largest difference on the others %.3g (%.2g of the band %.3g)" % (what, bad.sum(), bad.size, flipped.sum(), err, err / band, band))
    assert bad.sum() <= T.max_outside(tag, bad.size), "%s: %d chains differ" % (what, bad.sum())
    if case is not None and a.h_old is not None:
        assert b.h_old is not None and a.h_old.shape == b.h_old.shape
        for name, x, y in (("H_old", a.h_old, b.h_old), ("H_new", a.h_new, b.h_new)):
            tol = np.where((np.arange(x.shape[0]) <= n0)[:, None], T.h_tol(tag, case, x), T.h_tol_loose(tag, case, x))
            share = (np.abs(x - y) / tol)[:, ~bad]
            print("%s: %s at %.2g of its tolerance up to trajectory %d, %.2g beyond" % (what, name, share[:n0 + 1].max(), n0, share[n0 + 1:].max()))
            assert np.isfinite(y).all() and (share <= 1.0).all(), "%s: %s differs by %.3g of its tolerance" % (what, name, share.max())
    return bad


RUNS = [r for r in T.runs() if r[0] != "big"]


@pytest.mark.parametrize("cid,route", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_trajectories_vs_oracle(cid, route):
    """Every table case on every route it names: the kernel the restated launcher names (the one asked for, or where a refusal lands),
    the energies of trajectory 0 on every chain, rows and cur chain by chain, and on the chains inside the band accept, reject_count,
    the acceptance rate and the reset row of burn + 1.  The launch-edge cases (C % 4 of the wave kernels, 63 | 64 | 65 chains of the
    one-chain-per-lane kernels, 15 | 16 | 17 of the quad kernel, 32 chains per block once) are rows of the same table."""
    case = T.CASES[cid]
    got = single(cid, route)
    against_oracle("%s %s %s" % (cid, route, got.routes[0]), route, case, got, T.reference(cid))


ENERGY_RUNS = [r for r in RUNS if T.ROUTES[r[1]].diag]


@pytest.mark.parametrize("cid,route", ENERGY_RUNS, ids=["%s-%s" % r for r in ENERGY_RUNS])
def test_energies_of_trajectory_0_vs_oracle(cid, route):
    """H_old and H_new of trajectory 0 on EVERY chain of every run that asks for them, no exemption: there is no decision before them.
    (Before eig_polish_kernel normalised the float32 Jacobi eigenvectors, hmc_gauss_wave_eig_kernel<float,R> missed this from D = 63 by
    1.5 - 3.0 tolerances on both energies, with every decision and row right: tests/gauss_traj_cases.py.)"""
    case = T.CASES[cid]
    got = single(cid, route)
    for what, (s, c, err) in energy_shares(route, case, got, T.reference(cid)).items():
        assert s <= 1.0, "%s %s %s: %s of trajectory 0 differs by %.3g on chain %d (%.3g of its tolerance)" % (cid, route, got.routes[0], what, err, c, s)


def test_a_launch_of_more_than_65535_workgroups():
    """4 x 65535 + 1 chains of D = 7 on the direct wave kernel - 65536 workgroups, the last with one live wave and three that shadow
    the last chain: every output written, and the first 4, the last 4 and 9 chains spread between against the oracle."""
    case = T.CASES["big"]
    got = launch(case, "wave")
    for a in (got.rows, got.cur, got.h_old, got.h_new):
        assert np.isfinite(a).all()
    assert (got.accept <= 1).all() and (got.rejected >= 0).all() and (got.rejected <= case.ntraj).all()
    assert np.array_equal(got.rejected, (got.accept == 0).sum(0))
    sub = got.chains(T.probe_chains(case))
    against_oracle("big wave", "wave", case, sub, T.reference("big"))
    for what, (s, c, err) in energy_shares("wave", case, sub, T.reference("big")).items():
        assert s <= 1.0, "big: %s of trajectory 0 at %.3g of its tolerance on probe chain %d" % (what, s, c)


CUTS = [(cid, r) for cid in T.CUT_IDS for r in T.CASES[cid].routes]


@pytest.mark.parametrize("cid,route", CUTS, ids=["%s-%s" % r for r in CUTS])
def test_two_launches_are_one(cid, route):
    """Two launches over traj_offset with the state travelling through cur, cut before, at and after trajectory burn + 1 (the second
    launch starts with the trajectory that may reset, with the one after it - from a state the reset wrote -, and one later).  On the
    kernel that carries only the point: the same bits as the single launch in the rows, cur, reject_count and every per-trajectory
    output.  On the others (tests/gauss_traj_cases.py: TWO LAUNCHES) and where the shorter launches leave the one-launch quad route: the
    same decisions, rows and cur inside the row band, and H_old / H_new of every trajectory within the energy tolerance (the
    trajectory-0 one up to the first trajectory of the second launch, the untightened one beyond), on the chains that kept their decisions.  Either way every launch lands where the restated rule says."""
    case = T.CASES[cid]
    one = single(cid, route)
    tag = T.tag(route)
    for n0 in (case.burn, case.burn + 1, case.burn + 2):
        two = launch(case, route, spans=[(0, n0), (n0, case.ntraj - n0)])
        what = "%s %s cut at %d" % (cid, route, n0)
        if all(T.carries_only_the_point(k) for k in one.routes + two.routes):
            same_bits(one, two, what)
        else:
            same_values(one, two, tag, T.row_band(tag, one.routes[0], case.D, one.rows), what, case, n0)
            against_oracle(what, route, case, two, T.reference(cid))
    b1 = T.reference(cid).accept[case.burn + 1]
    assert b1.any() and (~b1).any()


PADS = [(cid, r) for cid in T.PAD_IDS for r in T.CASES[cid].routes]


@pytest.mark.parametrize("cid,route", PADS, ids=["%s-%s" % r for r in PADS])
def test_rows_behind_the_last_chain_are_not_touched(cid, route):
    """Five rows of 1e6 behind the last chain of cur and theta_init (C unchanged; the dead waves of the wave kernels shadow chain
    C - 1, the dead lanes of the others read nothing): the same bits in every output, the extra rows and the entries behind
    reject_count as they were."""
    one = single(cid, route)
    padded = launch(T.CASES[cid], route, pad=5)
    assert padded.routes == one.routes
    same_bits(one, padded, "%s %s padded" % (cid, route))


@pytest.mark.parametrize("cid", ["r3b7", "w7b7", "r3b0", "w7b0"])
def test_burn_in_rows_are_not_written(cid):
    """burn = T - 1: every trajectory is burn-in, the sample buffer is row 0 alone and is not written (launch() holds it to a sentinel and the rows
    around it to NaN) while cur and reject_count move as the oracle's do; burn = 0: trajectory 0 writes no row, trajectory 1 is the reset."""
    case = T.CASES[cid]
    ref = T.reference(cid)
    for route in case.routes:
        got = single(cid, route)
        assert got.rows.shape[0] == case.ntraj - case.burn
        moved = np.abs(got.cur - got.theta0).max(axis=1) > 0
        assert np.array_equal(moved, np.abs(ref.cur - ref.theta0).max(axis=1) > 0) and moved.any()


PAIRS = [(c.id, a, b) for c in T.TABLE for a, b in (("small_ws", "small_inline"), ("wave_eig", "wave"), ("wave_eig_f64", "wave_f64"), ("small_ws_f64", "small_inline_f64"))
         if a in c.routes and b in c.routes and c.id != "big"]


@pytest.mark.parametrize("cid,a,b", PAIRS, ids=["%s-%s" % p[:2] for p in PAIRS])
def test_same_draws_on_both_forms(cid, a, b):
    """The pre-drawn records against the draws made inside the kernel, and the eigenbasis wave kernel against the direct one (where a
    case reaches both): the same Philox draws, so the same decisions on every chain and the same values inside the row band."""
    case = T.CASES[cid]
    x, y = single(cid, a), single(cid, b)
    tag = T.tag(a)
    band = max(T.row_band(tag, k, case.D, y.rows) for k in x.routes + y.routes)
    bad = same_values(x, y, tag, band, "%s %s against %s" % (cid, x.routes[0], y.routes[0]))
    if x.routes == y.routes:          # a refusal landed on the same kernel: then the same bits
        same_bits(x, y, "%s %s and %s" % (cid, a, b))
    elif a.startswith("small_ws"):      # the same arithmetic behind two sources of the same draws
        assert not bad.any()


@pytest.mark.parametrize("cid", ["m7f", "m65f"])
def test_a_dense_mass_on_the_eigenbasis_shapes_takes_the_direct_kernel(cid):
    """Identity-mass shapes of hmc_gauss_wave_eig_kernel (D <= 128, a workspace) with a dense mass: the direct kernel, its lower-
    triangular momentum draw, against the oracle; the workspace it was handed changes no bit."""
    case = T.CASES[cid]
    got = single(cid, "wave_eig")
    assert got.routes == ["hmc_gauss_wave_kernel<float,%d,2>" % T.wave_r(case.D)]
    against_oracle("%s wave_eig" % cid, "wave_eig", case, got, T.reference(cid))
    assert all(s <= 1.0 for s, _, _ in energy_shares("wave_eig", case, got, T.reference(cid)).values())
    same_bits(got, single(cid, "wave"), "%s with and without a workspace" % cid)
