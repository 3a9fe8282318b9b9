"""GPU parity of the explicit-RMHMC kernels for Gaussian targets in TRAJECTORY mode - rmhmc_fused_kernel<T,KH,1|2,tracked>,
rmhmc_fused_kernel_wide<56|64>, rmhmc_mfma4_kernel, rmhmc_batch_kernel<25|28> (hamiltorch_amd/csrc/rmhmc_fused.hip and the
rmhmc_fused_*_dev.hpp it includes), rmhmc_uv_kernel<G,
co|solo> (rmhmc_uv.hip), rmhmc_uvc_kernel and rmhmc_uvc2_kernel (rmhmc_uvc.hip), behind the three momentum kernels - against
oracle/hmc_oracle.py:sample_rmhmc_explicit in float64 on the same Philox draws, through _abi.rmhmc_gaussian_sample directly: cur,
theta_init, the workspace, H_old / H_new / accept / reject_count, traj_offset and chain_offset are the test's.  Cases, reference,
bounds and the launcher's rules restated: tests/rmhmc_traj_cases.py; that every case discriminates (its step size makes the oracle
reject): tests/test_rmhmc_traj_cases_cpu.py.

Every launch asserts _abi.last_route() against the restated rule, so no run compares a kernel with itself or lands on another one
silently.  Trajectory 0 has no Metropolis decision before it, so its two energies are held to the oracle's on EVERY chain: H_old pins
the draw indices, the momentum law, both log-determinants' first use, the kinetic term and log p with its mean and log_norm, H_new the
whole step loop on top.  The rows, `cur`, accept, reject_count and the Q2 reset row pin everything the trajectory shells share."""
import functools

import numpy as np
import pytest
import torch

import rmhmc_traj_cases as T

pytestmark = pytest.mark.gpu
OUTPUTS = ("rows", "cur", "rejected", "h_old", "h_new", "accept")
CUT_ROUTES = ("fused_t", "fused_e", "wide_t", "pair2", "uv1_co", "uv2_solo", "uvc_co", "uvc_solo", "uvc2_co", "uvc2_solo", "mfma4_t", "mfma4_e",
              "batch_t", "batch_e")


def dev():
    return torch.device("cuda:0")


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Out:
    """What one or several launches left: rows[T - burn, C, D], cur[C, D], rejected[C], h_old / h_new / accept[T, C], routes."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def chains(self, sel):
        return Out(rows=self.rows[:, sel], cur=self.cur[sel], rejected=self.rejected[sel], h_old=self.h_old[:, sel], h_new=self.h_new[:, sel],
                   accept=self.accept[:, sel], theta0=self.theta0[sel], routes=self.routes)


def launch(case, route, spans=None, pad=0, min_workspace=False):
    """The trajectories of `case` under the tuning keys of `route`, one launch per (traj_offset, n_traj) span (default: one launch for
    all), the state travelling through `cur`.  pad: that many rows of 1e6 behind the last chain in cur and theta_init (and untouched
    entries behind reject_count), C unchanged.  min_workspace: no room beyond the base layout.  Unwritten outputs stay NaN / 255."""
    from hamiltorch_amd import _abi
    dtype = torch.float64 if route == "f64" else torch.float32
    P, mu = T.inputs_of(case.D)
    C, D, n_rows = case.C, case.D, case.ntraj - case.burn
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev())
    Pd, mud = t(P), t(mu)
    init_all = torch.full((C + pad, D), 1e6, dtype=dtype, device=dev())
    init_all[:C] = t(T.starts(case))
    cur_all = init_all.clone()
    theta0, cur = init_all[:C], cur_all[:C]
    rows = torch.full((n_rows, C, D), float("nan"), dtype=dtype, device=dev())
    rows[0] = theta0
    rej_all = torch.full((C + pad,), -7, dtype=torch.int32, device=dev())
    rej_all[:C] = 0
    ws = torch.empty(_abi.rmhmc_workspace_bytes(C, D, Pd.element_size(), 0 if min_workspace else case.ntraj), dtype=torch.uint8, device=dev())
    ho, hn, ac, routes = [], [], [], []
    try:
        for k, v in T.ROUTES[route].items():
            _abi.set_tuning(k, v)
        for k, v in dict(T.DEFAULT_KEYS, **T.ROUTES[route]).items():
            assert _abi.get_tuning(k) == v, (k, v, _abi.get_tuning(k))
        for n0, cnt in spans or [(0, case.ntraj)]:
            Ho = torch.full((cnt, C), float("nan"), dtype=dtype, device=dev())
            Hn = torch.full_like(Ho, float("nan"))
            acc = torch.full((cnt, C), 255, dtype=torch.uint8, device=dev())
            _abi.rmhmc_gaussian_sample(cur, theta0, Pd, mud, T.log_norm(D), _abi.METRIC_SOFTABS, T.ALPHA, case.jitter, case.L, case.eps, T.OMEGA,
                                       cnt, n0, case.burn, case.seed, T.CHAIN_OFFSET, rows, rej_all[:C], ws, H_old=Ho, H_new=Hn, accept=acc)
            routes.append(_abi.last_route())
            ho.append(Ho); hn.append(Hn); ac.append(acc)
        torch.cuda.synchronize()
    finally:
        _abi.reset_tuning()
    if pad:
        assert bool((init_all[C:] == 1e6).all()) and bool((cur_all[C:] == 1e6).all()) and bool((rej_all[C:] == -7).all())
    n = lambda x: x.cpu().numpy()
    return Out(rows=n(rows), cur=n(cur), rejected=n(rej_all[:C]), h_old=n(torch.cat(ho)), h_new=n(torch.cat(hn)), accept=n(torch.cat(ac)),
               routes=routes, theta0=n(theta0))


@functools.lru_cache(maxsize=None)
def single(cid, route):
    """One launch for all trajectories of a table case on a route: run once, shared by the tests that compare with it."""
    return launch(T.CASES[cid], route)


def against_oracle(name, tag, case, got, ref):
    """The assertions of a run against its oracle (tests/rmhmc_traj_cases.py: BOUNDS); prints the figures it asserts on."""
    for a in (got.rows, got.cur, got.h_old, got.h_new):
        assert np.isfinite(a).all(), "%s: an output was not written (or is not finite)" % name
    assert set(np.unique(got.accept)) <= {0, 1}
    n_c = got.cur.shape[0]
    # trajectory 0: every chain, no exemption
    share = {}
    for what, g, w in (("H_old", got.h_old[0], ref.h_old[0]), ("H_new", got.h_new[0], ref.h_new[0])):
        s = np.abs(g - w) / T.h_tol(tag, w)
        share[what] = (s.max(), int(s.argmax()), np.abs(g - w).max())
    band = T.row_band(tag, ref.rows)
    out = T.outside(got.rows.astype(np.float64), got.cur.astype(np.float64), ref, band)
    inside = ~out
    err_in = max(np.abs(got.rows - ref.rows)[:, inside].max(), np.abs(got.cur - ref.cur)[inside].max()) if inside.any() else np.nan
    b1 = case.burn + 1
    print("%s: oracle acceptance %.2f%s; trajectory 0 H_old at %.2g, H_new at %.2g of their tolerance; %d of %d chains outside the row band of %.3g, "
          "largest difference inside %.3g (%.2g of the band)" % (name, ref.accept.mean(), ", %d rejects at burn + 1" % (~ref.accept[b1]).sum() if 0 <= b1 < case.ntraj else "",
                                                                share["H_old"][0], share["H_new"][0], out.sum(), n_c, band, err_in, err_in / band))
    for what, (s, c, err) in share.items():
        assert s <= 1.0, "%s: %s of trajectory 0 differs by %.3g on chain %d (%.3g of its tolerance)" % (name, what, err, c, s)
    assert out.sum() <= T.max_outside(tag, n_c), "%s: %d of %d chains outside the band, max err %.3g" % (name, out.sum(), n_c, np.nanmax(np.abs(got.rows - ref.rows)))
    # on the chains inside the band: the decisions, their count, the acceptance rate, the Q2 reset, the state handed back
    assert np.array_equal(got.accept[:, inside].astype(bool), ref.accept[:, inside]), "%s: accept differs" % name
    assert np.array_equal(got.rejected[inside], ref.rejected[inside]), "%s: reject_count differs" % name
    assert np.array_equal(1.0 - got.rejected[inside] / float(case.ntraj), ref.acc_rate[inside])
    if 0 <= b1 < case.ntraj:
        reset = inside & ~ref.accept[b1]
        assert np.array_equal(got.rows[1][reset], got.theta0[reset]), "%s: the row of burn + 1 of a rejecting chain is not theta_init" % name
    if case.ntraj - 1 > case.burn:
        assert np.array_equal(got.cur, got.rows[-1]), "%s: the state handed back is not the last row" % name
    assert np.array_equal(got.rows[0], got.theta0)


def same_bits(a, b, what):
    for k in OUTPUTS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), "%s: %s differs" % (what, k)


def law_of(case, route, reported):
    """tests/test_gpu_rmhmc.py:oracle_momentum."""
    from hamiltorch_amd import _abi
    if reported.startswith("rmhmc_"):
        return T.momentum_law(case, route)
    return "sqrt" if reported in ("metric_traj_mfma_kernel", "metric_warm_mfma_kernel") and _abi.get_tuning("metric_sqrtdraw") else "chol"


RUNS = T.runs()


@pytest.mark.parametrize("cid,route", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_trajectories_vs_oracle(cid, route):
    """Every table case under the keys of every route: the kernel the restated launcher names (the one asked for, or where a refusal
    lands; D = 129 leaves the family), the energies of trajectory 0 on every chain, rows and cur chain by chain, and on the chains
    inside the band accept, reject_count, the acceptance rate and the reset row of burn + 1."""
    case = T.CASES[cid]
    got = single(cid, route)
    want = T.expected_route(case, route, cus())
    if want is None:
        assert case.D > T.FAMILY_D and not got.routes[0].startswith("rmhmc_"), got.routes
    else:
        assert got.routes == [want], (got.routes, want)
    against_oracle("%s %s %s" % (cid, route, got.routes[0]), T.tag(route), case, got, T.reference(cid, law_of(case, route, got.routes[0])))


def test_momentum_kernels_draw_the_law_asked_for():
    """The split draw, the wave draw and the workgroup draw behind the same one-chain kernel on one case: the first follows another
    law than the other two (other momenta from the same streams), the wave and the workgroup draw the same momenta in another order
    of sums."""
    cid = T.MOMENTUM_ID
    split, wave, wg = single(cid, "fused_t"), single(cid, "mom_wave"), single(cid, "mom_wg")
    assert split.routes == wave.routes == wg.routes == [T.expected_route(T.CASES[cid], "fused_t", cus())]
    assert T.momentum_law(T.CASES[cid], "fused_t") == "split" and T.momentum_law(T.CASES[cid], "mom_wave") == "chol" == T.momentum_law(T.CASES[cid], "mom_wg")
    a, b = T.reference(cid, "split"), T.reference(cid, "chol")
    tol = T.h_tol("f32", a.h_old[0])
    # the two laws are told apart: their H_old of trajectory 0 differ by more than twice the tolerance on most chains, in the oracle
    # and in the kernels alike (at jitter 1e-3 the two momenta of a chain are close: the same z through chol(P) and through chol(G))
    assert (np.abs(a.h_old[0] - b.h_old[0]) > 2 * tol).mean() > 0.8 and (np.abs(split.h_old[0] - wave.h_old[0]) > 2 * tol).mean() > 0.8
    assert (np.abs(wave.h_old[0] - wg.h_old[0]) <= 2 * tol).all() and not np.array_equal(wave.h_new, wg.h_new)


CUTS = [(cid, r) for cid in T.CUT_IDS for r in CUT_ROUTES + (("f64",) if cid in T.F64_IDS else ()) if (cid, r) in RUNS]


@pytest.mark.parametrize("cid,route", CUTS, ids=["%s-%s" % r for r in CUTS])
def test_two_launches_are_one(cid, route):
    """Two launches over traj_offset with the state travelling through cur, cut before, at and after trajectory burn + 1 (the second
    launch starts with the trajectory that may reset, with the one after it - from a state the reset wrote -, and one later): the same
    bits as the single launch in the rows, cur, reject_count and every per-trajectory output."""
    case = T.CASES[cid]
    one = single(cid, route)
    for n0 in (case.burn, case.burn + 1, case.burn + 2):
        two = launch(case, route, spans=[(0, n0), (n0, case.ntraj - n0)])
        assert two.routes == one.routes * 2
        same_bits(one, two, "%s %s cut at %d" % (cid, route, n0))
    assert (one.accept[case.burn + 1] == 0).any() and (one.accept[case.burn + 1] == 1).any()


PADS = [("k2", r) for r in T.F32_ROUTES if ("k2", r) in RUNS] + [("d7", "f64"), ("w2", "fused_t"), ("d128", "wide_t"), ("d112", "batch_t")]


@pytest.mark.parametrize("cid,route", PADS, ids=["%s-%s" % r for r in PADS])
def test_rows_behind_the_last_chain_are_not_touched(cid, route):
    """Five rows of 1e6 behind the last chain of cur and theta_init (C unchanged; C is odd, so the last workgroup of every two-, four-
    and sixteen-chain kernel is partial and its dead columns read something): the same bits in every output, the extra rows and the
    entries behind reject_count as they were."""
    one = single(cid, route)
    padded = launch(T.CASES[cid], route, pad=5)
    assert padded.routes == one.routes
    same_bits(one, padded, "%s %s padded" % (cid, route))


@pytest.mark.parametrize("cid,route", [("k2", "fused_t"), ("k2", "uvc_co"), ("w2", "fused_t"), ("k0", "uv2_co"), ("d100", "batch_t"), ("d7", "f64")])
def test_the_minimum_workspace_runs_in_passes(cid, route):
    """A workspace of rmhmc_workspace_bytes(C, D, itemsize, 0): the momentum kernels borrow the augmented-state area, four trajectories
    per pass - the same kernel (pre-drawn momenta, not a draw inside it) and the same bits as one pass of eight."""
    one = single(cid, route)
    two = launch(T.CASES[cid], route, min_workspace=True)
    assert two.routes == one.routes
    same_bits(one, two, "%s %s in passes of four" % (cid, route))


@pytest.mark.parametrize("name", sorted(T.edge_sizes(T.NOMINAL_CUS)))
def test_launch_edges_vs_oracle(name):
    """D = 3 at the chain counts where the launch changes: C = CUs and CUs + 1 (one chain per workgroup, then two), 2 CUs + 1, 7 CUs and
    7 CUs + 1 (the default route leaves the column kernels), and one chain past the grid of the one-chain kernel (8192 workgroups), of
    rmhmc_mfma4_kernel (4 x 8192 chains) and of rmhmc_batch_kernel (16 x 4096): the route from the restated rule, then the first 4, the
    last 4 and 9 chains spread between against the oracle."""
    n = cus()
    C, route = T.edge_sizes(n)[name]
    case = T.edge_case(C)
    got = launch(case, route)
    want = T.expected_route(case, route, n)
    assert got.routes == [want], (got.routes, want)
    per, grid, last = T.groups(want, C)
    print("%s: C = %d on %s: %d chains per workgroup, %d workgroups, %d in the last group" % (name, C, want, per, grid, last))
    for a in (got.rows, got.cur, got.h_old, got.h_new):
        assert np.isfinite(a).all()
    assert (got.accept <= 1).all() and (got.rejected >= 0).all() and (got.rejected <= case.ntraj).all()
    against_oracle("%s %s" % (case.id, want), "f32", case, got.chains(T.edge_chains(C)), T.reference(case.id, "split"))
