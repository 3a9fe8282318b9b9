"""No GPU: everything tests/test_gpu_rmhmc_traj.py takes for granted about tests/rmhmc_traj_cases.py, checked on the oracle alone - the
table covers the edges it was written for, the launcher's rules restated there give the K, `series` and kernel every case claims, and
every case can tell a wrong kernel from a right one: the oracle rejects and accepts, the Q2 reset at trajectory burn + 1 runs and is
told apart from "keep current", the mean and the jitter matter, the float32 arithmetic alone stays well inside the float32 bounds,
and a float64 decision has room."""
import numpy as np
import pytest

import rmhmc_traj_cases as T

EDGES = {name: T.edge_case(C) for name, (C, _) in T.edge_sizes(T.NOMINAL_CUS).items()}
EDGE_ROUTE = {name: r for name, (_, r) in T.edge_sizes(T.NOMINAL_CUS).items()}


def _ref(case, law):
    return T.reference(case.id, law)


def _chains(case):
    return T.edge_chains(case.C) if case.id.startswith("edge@") else None


def _leaves(side, ref, tag):
    """What the GPU test would notice of `side` in place of `ref`: an energy of trajectory 0 beyond its tolerance on any chain (no
    exemption there), a flipped decision or a row outside the band on more chains than the band exempts."""
    n = side.accept.shape[0]
    h = max((np.abs(side.h_old[0] - ref.h_old[0]) / T.h_tol(tag, ref.h_old[0])).max(), (np.abs(side.h_new[0] - ref.h_new[0]) / T.h_tol(tag, ref.h_new[0])).max())
    rows = min(side.rows.shape[0], ref.rows.shape[0])
    with np.errstate(invalid="ignore"):
        far = ~(np.abs(side.rows[:rows] - ref.rows[:rows]).max(axis=(0, 2)) <= T.row_band(tag, ref.rows))
    bad = far | (side.accept != ref.accept[:n]).any(axis=0)
    return h > 1.0 or bad.sum() > T.max_outside(tag, bad.size), "energies of trajectory 0 at %.3g of their tolerance, %d of %d chains differ" % (h, bad.sum(), bad.size)


def discriminates(case, law, f64=False, report=print):
    """The conditions of this module on one case under one momentum law; AssertionError where one fails."""
    chains = _chains(case)
    ref = T.run_oracle(case, law, chains) if case.id not in T.ALL_CASES or T.ALL_CASES[case.id] != case else _ref(case, law)
    name = "%s/%s" % (case.id, law)
    n_c = ref.accept.shape[1]
    assert np.isfinite(ref.rows).all() and np.isfinite(ref.h_old).all() and np.isfinite(ref.h_new[0]).all() and np.isfinite(ref.cur).all()
    rate = ref.accept.mean()
    b1 = case.burn + 1
    report("%s: eps %g, seed %d, acceptance %.2f%s" % (name, case.eps, case.seed, rate,
                                                      ", %d of %d chains reject at burn + 1" % ((~ref.accept[b1]).sum(), n_c) if 0 <= b1 < case.ntraj else ""))
    assert 0.2 <= rate <= 0.9, "%s: acceptance %.2f" % (name, rate)
    assert np.array_equal(ref.rejected, (~ref.accept).sum(0)) and np.allclose(ref.acc_rate, 1.0 - ref.rejected / case.ntraj)
    band = T.row_band("f32", ref.rows)
    if 0 <= b1 < case.ntraj:
        q2 = ref.accept[b1]
        assert q2.any() and (~q2).any(), "%s: %d accept at burn + 1" % (name, q2.sum())
        assert np.array_equal(ref.rows[1][~q2], ref.theta0[~q2].astype(np.float64))          # the row of burn + 1 of a rejecting chain is theta_init
        if case.burn >= 0:          # (at burn = -1 the reset row IS the point trajectory 0 starts from: nothing to tell apart)
            moved = np.abs(ref.starts[b1] - ref.theta0).max(axis=1)
            report("%s: rejecting chains started burn + 1 up to %.3g from theta_init (band %.3g)" % (name, moved[~q2].max(), band))
            assert (moved[~q2] > 100 * band).any(), "%s: no reset to tell from keeping the current point" % name
    assert ref.rejected.max() > ref.rejected.min()
    # the mean matters
    side = T.run_oracle(case, law, chains, mean=None, ntraj=1)
    hit, what = _leaves(side, ref, "f32")
    assert hit, "%s without the mean: %s" % (name, what)
    # the jitter matters where it is on (in float64 where only the float64 kernel can tell: jitter 1e-6)
    if case.jitter is not None:
        jt = "f64" if case.jitter < 1e-5 else "f32"
        hit, what = _leaves(T.run_oracle(case, law, chains, jitter=None, ntraj=1), ref, jt)
        if not hit:
            hit, what = _leaves(T.run_oracle(case, law, chains, jitter=None), ref, jt)
        report("%s without jitter (%s bounds): %s" % (name, jt, what))
        assert hit, "%s without jitter: %s" % (name, what)
    # float32 arithmetic alone: a third of every float32 bound
    low = T.run_oracle(case, law, chains, dtype=np.float32)
    assert low.rows.dtype == np.float32
    h = max((np.abs(low.h_old[0] - ref.h_old[0]) / T.h_tol("f32", ref.h_old[0])).max(), (np.abs(low.h_new[0] - ref.h_new[0]) / T.h_tol("f32", ref.h_new[0])).max())
    bad = T.outside(low.rows.astype(np.float64), low.cur.astype(np.float64), ref, band / 3) | (low.accept != ref.accept).any(axis=0)
    ok = ~bad
    report("%s: float32 oracle: energies of trajectory 0 at %.2g of their tolerance, %d of %d chains outside a third of the band or flipped; largest "
           "difference on the others %.3g (band %.3g)" % (name, h, bad.sum(), n_c, np.abs(low.rows - ref.rows)[:, ok].max() if ok.any() else np.nan, band))
    assert h <= 1.0 / 3.0 and bad.sum() <= T.max_outside("f32", n_c), "%s: float32 oracle: energies %.2g, %d chains" % (name, h, bad.sum())
    margin = T.guard_margin(ref)
    report("%s: closest decision %.3g max(1, |H|), |H| up to %.4g" % (name, margin.min(), np.abs(ref.h_old).max()))
    if f64:
        assert margin.min() >= T.GUARD, "%s: a decision %.3g from its threshold" % (name, margin.min())
    return ref


def test_the_table_covers_the_edges_asked_for():
    C = T.CASES
    assert all(c.C <= 32 and 2 <= c.L <= 3 and c.ntraj == 8 for c in T.ALL_CASES.values() if not c.id.startswith("edge@"))
    assert all(c.C <= 12 for c in T.TABLE if c.D >= 97)
    assert all(c.burn == 2 for c in T.TABLE if c.id not in ("bm1", "b0", "b7"))
    assert {c.burn for c in T.TABLE if c.D == 7 and c.jitter == 1e-3} == {-1, 0, 2, T.NTRAJ - 1}
    assert {1, 3, 7, 31, 32, 33, 64, 65, 97, 100, 101, 112, 113, 128, 129} <= {c.D for c in T.TABLE}
    # refinement counts with the series: K = 0, 1, 2, 3; the in-kernel Cholesky: series = 0
    assert [T.fused_plan(C[k].D, C[k].jitter) for k in ("k0", "k1", "k2", "k3")] == [(0, 1), (1, 1), (2, 1), (3, 1)]
    assert [T.fused_plan(C[k].D, C[k].jitter) for k in ("w2", "w5")] == [(3, 0), (7, 0)]
    assert (C["k0"].jitter, C["k1"].jitter, C["k2"].jitter, C["k3"].jitter, C["w2"].jitter, C["w5"].jitter) == (None, 6e-5, 1e-3, 1.3e-3, 2e-3, 5e-2)
    # float64: jitter 1e-6 the series form, 1e-3 the Cholesky form, at D = 7, 33, 100
    assert sorted(C[k].D for k in T.F64_IDS) == [7, 7, 33, 33, 100, 100]
    for k in T.F64_IDS:
        K, series = T.fused_plan(C[k].D, C[k].jitter, f64=True)
        assert (C[k].jitter, series, K) in ((1e-6, 1, 2), (1e-3, 0, 6)), (k, K, series)
    # an odd C on every two-chain form, a C not divisible by 4 / 16 on mfma4 / batch
    assert all(c.C % 2 == 1 for c in T.TABLE)
    # both KH values of the wide instances
    assert T.kh(100) == 56 and T.kh(128) == 64 and T.kh(97) == 56 and T.kh(113) == 64 and T.kh(96) == 48
    # the launch-edge sizes
    n = T.NOMINAL_CUS
    assert {k: v[0] for k, v in T.edge_sizes(n).items()} == {"cus": n, "cus+1": n + 1, "2cus+1": 2 * n + 1, "7cus": 7 * n, "7cus+1": 7 * n + 1,
                                                           "one+1": 8193, "mfma4+1": 4 * 8192 + 1, "batch+1": 16 * 4096 + 1}
    for c in EDGES.values():
        sel = T.edge_chains(c.C)
        assert c.D == 3 and list(sel[:4]) == [0, 1, 2, 3] and list(sel[-4:]) == list(range(c.C - 4, c.C)) and np.all(np.diff(sel) > 0)


def test_the_restated_launcher_sends_every_case_where_it_claims():
    """Every kernel of the family is reached, by the cases that may reach it; a refused case lands on the kernel named here."""
    C, n = T.CASES, T.NOMINAL_CUS
    seen = {}
    for cid, route in T.runs():
        name = T.expected_route(C[cid], route)
        seen.setdefault(name.split("<")[0] if name else None, set()).add(cid)
        if cid == "d129":
            assert name is None
            continue
        assert name.startswith("rmhmc_")
        K, series = T.fused_plan(C[cid].D, C[cid].jitter, route == "f64")
        lean = series or C[cid].jitter is None
        if route == "default":          # 9 .. 31 chains: the column kernels where they take the case, else the one-chain kernel
            assert name.split("<")[0] in ("rmhmc_uv_kernel", "rmhmc_uvc_kernel") if lean and C[cid].D <= 100 else name.startswith("rmhmc_fused_kernel")
            continue
        takes = name.startswith(T.ASKS_FOR[route])
        if route in ("uv1_co", "uv1_solo", "uv2_co", "uv2_solo", "uvc2_co", "uvc2_solo", "mfma4_t", "mfma4_e"):
            assert takes == bool(lean and C[cid].D <= 100), (cid, route, name)
        elif route in ("uvc_co", "uvc_solo"):
            assert takes == bool(lean and C[cid].D <= 100 and K == 2 and C[cid].jitter is not None), (cid, route, name)
            if lean and C[cid].D <= 100 and not takes:
                assert name.startswith("rmhmc_uv_kernel<1,")
        elif route in ("batch_t", "batch_e"):
            assert takes == bool(lean and C[cid].D <= 112), (cid, route, name)
        elif route == "pair2":
            assert name.endswith(",2>") == bool(lean)
        elif route in ("wide_t", "wide_e"):
            assert takes and name.startswith("rmhmc_fused_kernel_wide<%d," % (56 if C[cid].D <= 112 else 64))
        elif route != "default":
            assert takes, (cid, route, name)
    assert set(seen) == {None, "rmhmc_fused_kernel", "rmhmc_fused_kernel_wide", "rmhmc_uv_kernel", "rmhmc_uvc_kernel", "rmhmc_uvc2_kernel",
                         "rmhmc_mfma4_kernel", "rmhmc_batch_kernel"}
    assert seen["rmhmc_uvc_kernel"] >= {"k2", "d1", "d100"} and not seen["rmhmc_uvc_kernel"] & {"k0", "k1", "k3", "w2", "w5", "d101"}
    assert seen["rmhmc_uv_kernel"] >= {"k0", "k1", "k2", "k3"}
    # the refusals by name
    assert T.expected_route(C["d101"], "uv1_co") == "rmhmc_fused_kernel_wide<56,true>" and T.expected_route(C["d101"], "mfma4_t") == "rmhmc_fused_kernel_wide<56,true>"
    assert T.expected_route(C["d101"], "batch_t") == "rmhmc_batch_kernel<28,true>" and T.expected_route(C["d100"], "batch_e") == "rmhmc_batch_kernel<25,false>"
    assert T.expected_route(C["d112"], "batch_t") == "rmhmc_batch_kernel<28,true>" and T.expected_route(C["d113"], "batch_t") == "rmhmc_fused_kernel_wide<64,true>"
    assert T.expected_route(C["w2"], "uv1_co") == "rmhmc_fused_kernel<float,24,1,true>" == T.expected_route(C["w2"], "pair2")
    assert T.expected_route(C["d128"], "fused_e") == "rmhmc_fused_kernel<float,64,1,false>" and T.expected_route(C["d128"], "wide_t") == "rmhmc_fused_kernel_wide<64,true>"
    assert T.expected_route(C["d100"], "f64") == "rmhmc_fused_kernel<double,56,1,false>"
    # the launch-edge sizes on their routes, and the groups of their grids
    want = {"cus": "rmhmc_uvc_kernel<co>", "cus+1": "rmhmc_uvc2_kernel<co>", "2cus+1": "rmhmc_uvc2_kernel<co>", "7cus": "rmhmc_uvc2_kernel<co>",
            "7cus+1": "rmhmc_mfma4_kernel<true>", "one+1": "rmhmc_fused_kernel<float,8,1,true>", "mfma4+1": "rmhmc_mfma4_kernel<true>",
            "batch+1": "rmhmc_batch_kernel<25,true>"}
    for k, c in EDGES.items():
        assert T.expected_route(c, EDGE_ROUTE[k], n) == want[k], k
    assert T.groups(want["one+1"], 8193) == (1, 8192, 1) and T.groups(want["mfma4+1"], 32769) == (4, 8192, 1) and T.groups(want["batch+1"], 65537) == (16, 4096, 1)
    assert T.groups(want["cus+1"], n + 1) == (2, n // 2 + 1, 1) and T.groups("rmhmc_fused_kernel<float,24,2>", 31) == (2, 16, 1)
    assert T.groups("rmhmc_mfma4_kernel<true>", 31)[2] == 3 and T.groups("rmhmc_batch_kernel<25,true>", 31)[2] == 15 and T.groups("rmhmc_batch_kernel<25,true>", 9)[2] == 9
    # at another CU count 7 cus + 1 need not be in mfma4's default range: the rule, not the name, is what the GPU test asserts
    assert T.expected_route(T.edge_case(7 * 304 + 1), "default", 304) == "rmhmc_batch_kernel<25,true>"


def test_the_inputs_are_the_ones_described():
    for c in T.TABLE:
        P, mu = T.inputs_of(c.D)
        lam = np.linalg.eigvalsh(P.astype(np.float64))
        assert P.dtype == mu.dtype == np.float32 and np.array_equal(P, P.T) and abs(lam.min() - 0.5) < 1e-5 and abs(lam.max() - (2.0 if c.D > 1 else 0.5)) < 1e-5
        assert np.array_equal(mu, np.linspace(-1, 1, c.D).astype(np.float32)) and np.abs(mu).max() == 1.0 and T.log_norm(c.D) != 0.0
        th0 = T.starts(c)
        assert th0.dtype == np.float32 and th0.shape == (c.C, c.D) and 0.05 < np.abs(th0 - mu).std() / 0.3 < 2.0
        assert np.array_equal(T.starts(c, [c.C - 1])[0], th0[-1])


@pytest.mark.parametrize("cid", [c.id for c in T.TABLE])
def test_every_case_discriminates(cid):
    """The float64 oracle alone, under every momentum law the case is run under: acceptance over chains x trajectories in [0.2, 0.9];
    at trajectory burn + 1 at least one chain accepts and one rejects, and a rejecting one had moved more than 100 row bands from
    theta_init (where burn + 1 exists; at burn = -1 the reset row is the start itself); the run with the mean at 0 and the run
    without jitter would be noticed; the oracle entirely in float32 stays within a third of every float32 bound and flips a decision
    on no more chains than the band exempts; on a float64 case no decision lies within GUARD max(1, |H|) of its threshold."""
    case = T.CASES[cid]
    for law in T.laws(case):
        ref = discriminates(case, law, cid in T.F64_IDS)
        assert ref.rows.shape == (case.ntraj - case.burn, case.C, case.D)


@pytest.mark.parametrize("name", sorted(EDGES))
def test_the_launch_edge_runs_discriminate(name):
    """The same conditions on the 17 compared chains of every launch-edge size at the nominal CU count."""
    case = EDGES[name]
    assert case.C in T.EDGE_STEPS
    discriminates(case, "split")
    assert T.max_outside("f32", 17) == 0 and T.max_outside("f32", 31) == 1 and T.max_outside("f32", 9) == 0 and T.max_outside("f64", 31) == 0
