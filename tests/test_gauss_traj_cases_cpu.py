"""No GPU: everything tests/test_gpu_gauss_traj.py takes for granted about tests/gauss_traj_cases.py, checked on the oracle alone - the
table reaches every kernel instance and every R, the launcher's rules restated there send every (case, route) where it claims and every
refusal where it is named, the workspace formula gives the hand-computed sizes, and every case can tell a wrong kernel from a right
one: the oracle rejects and accepts, the Q2 reset at trajectory burn + 1 runs and is told apart from "keep current", the mean, log_norm
and the mass operand matter, a draw indexed by t instead of traj_offset + t shows on the two-launch cases, the float32 arithmetic alone
stays within a third of every float32 bound without flipping a decision, and a float64 decision has room.

`python tests/test_gauss_traj_cases_cpu.py [ids]` runs the search of tests/gauss_traj_cases.py:search over the conditions below and
prints the STEPS and H_DIST entries."""
import math
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_root, "oracle"), os.path.join(_root, "tests")]

import gauss_traj_cases as T


def _tags(case):
    return sorted({T.tag(r) for r in case.routes})


def _bands(case, ref, tag):
    """The row bands of the case's routes of a dtype (a case may land on a register-resident kernel and on a wave kernel)."""
    return sorted({T.row_band(tag, T.expected_route(case, r), case.D, ref.rows) for r in case.routes if T.tag(r) == tag})


def _leaves(side, ref, case, tag, band, dist):
    """What the GPU test would notice of `side` in place of `ref`: an energy of trajectory 0 beyond its tolerance on any chain (no
    exemption there), a flipped decision or a row outside the band on more chains than the band exempts."""
    n = side.accept.shape[0]
    h = max((np.abs(side.h_old[0] - ref.h_old[0]) / T.h_tol(tag, case, ref.h_old[0], dist)).max(),
            (np.abs(side.h_new[0] - ref.h_new[0]) / T.h_tol(tag, case, ref.h_new[0], dist)).max())
    rows = min(side.rows.shape[0], ref.rows.shape[0])
    with np.errstate(invalid="ignore"):
        far = ~(np.abs(side.rows[:rows] - ref.rows[:rows]).max(axis=(0, 2)) <= band)
    bad = far | (side.accept != ref.accept[:n]).any(axis=0)
    return h > 1.0, bad.sum() > T.max_outside(tag, bad.size), "energies of trajectory 0 at %.3g of their tolerance, %d of %d chains differ" % (h, bad.sum(), bad.size)


def discriminates(case, report=print):
    """The conditions of this module on one case; AssertionError where one fails.  Returns the float64 reference."""
    recorded = case.id in T.CASES and T.CASES[case.id] == case and case.id in T.H_DIST
    ref = T.reference(case.id) if recorded else T.run_oracle(case)
    dist = None if recorded else _round_up(T.h_distance(case))
    name = case.id
    n_c = ref.accept.shape[1]
    assert np.isfinite(ref.rows).all() and np.isfinite(ref.h_old).all() and np.isfinite(ref.h_new).all() and np.isfinite(ref.cur).all()
    rate = ref.accept.mean()
    b1 = case.burn + 1
    report("%s: f %.2f, eps %.4f, seed %d, acceptance %.2f%s" % (name, case.f, T.eps_of(case), case.seed, rate,
                                                                ", %d of %d chains reject at burn + 1" % ((~ref.accept[b1]).sum(), n_c) if 0 <= b1 < case.ntraj else ""))
    assert 0.2 <= rate <= 0.9, "%s: acceptance %.2f" % (name, rate)
    assert np.array_equal(ref.rejected, (~ref.accept).sum(0)) and np.allclose(ref.acc_rate, 1.0 - ref.rejected / case.ntraj)
    tags = _tags(case)
    widest = max(b for t in tags for b in _bands(case, ref, t))
    if 0 <= b1 < case.ntraj:
        q2 = ref.accept[b1]
        assert q2.any() and (~q2).any(), "%s: %d accept at burn + 1" % (name, q2.sum())
        assert np.array_equal(ref.rows[1][~q2], ref.theta0[~q2].astype(np.float64))          # the row of burn + 1 of a rejecting chain is theta_init
        if case.burn >= 0:          # (at burn = -1 the reset row IS the point trajectory 0 starts from: nothing to tell apart)
            moved = np.abs(ref.starts[b1] - ref.theta0).max(axis=1)
            report("%s: rejecting chains started burn + 1 up to %.3g from theta_init (widest band %.3g)" % (name, moved[~q2].max(), widest))
            assert (moved[~q2] > 100 * widest).any(), "%s: no reset to tell from keeping the current point" % name
    assert ref.rejected.max() > ref.rejected.min()
    # the mean, log_norm and the mass operand matter: each alone moves an energy of trajectory 0 beyond its tolerance, under every dtype's
    for tag in tags:
        for what, kw in (("the mean", dict(mean=None)), ("log_norm", dict(lognorm=None))) + ((("the mass operand", dict(mass=None)),) if case.mass != "none" else ()):
            hit, _, text = _leaves(T.run_oracle(case, ntraj=1, **kw), ref, case, tag, widest, dist)
            assert hit, "%s without %s (%s): %s" % (name, what, tag, text)
    # a draw indexed by t instead of traj_offset + t, on the two-launch cases: the rows (or a decision) show it
    if case.id in T.CUT_IDS:
        for n0 in (case.burn, case.burn + 1, case.burn + 2):
            _, hit, text = _leaves(T.run_oracle(case, restart_at=n0), ref, case, "f32", widest, dist)
            assert hit, "%s with the second launch's draws restarted at %d: %s" % (name, n0, text)
    # float32 arithmetic alone: a third of every float32 bound, no decision flipped
    low = T.run_oracle(case, dtype=np.float32)
    assert low.rows.dtype == np.float32
    h = max((np.abs(low.h_old[0] - ref.h_old[0]) / T.h_tol("f32", case, ref.h_old[0], dist)).max(),
            (np.abs(low.h_new[0] - ref.h_new[0]) / T.h_tol("f32", case, ref.h_new[0], dist)).max())
    tight = min(_bands(case, ref, "f32"))
    far = T.outside(low.rows.astype(np.float64), low.cur.astype(np.float64), ref, tight / 3)
    flipped = (low.accept != ref.accept).any(axis=0)
    report("%s: float32 oracle: energies of trajectory 0 at %.2g of their tolerance, %d of %d chains outside a third of the band %.3g, %d flipped; "
           "largest difference %.3g" % (name, h, far.sum(), n_c, tight, flipped.sum(), np.abs(low.rows - ref.rows).max()))
    assert h <= 1.0 / 3.0 and not far.any() and not flipped.any(), "%s: float32 oracle: energies %.2g, %d chains far, %d flipped" % (name, h, far.sum(), flipped.sum())
    margin = T.guard_margin(ref)
    report("%s: closest decision %.3g max(1, |H|), |H| up to %.4g" % (name, margin.min(), np.abs(ref.h_old).max()))
    if "f64" in tags:
        assert margin.min() >= T.GUARD, "%s: a decision %.3g from its threshold" % (name, margin.min())
    return ref


def _round_up(x):
    """x rounded up to two significant digits."""
    e = 10.0 ** (math.floor(math.log10(x)) - 1)
    return float("%.2g" % (math.ceil(x / e) * e))


def test_the_table_covers_the_cases_asked_for():
    C = T.CASES
    small = [c for c in T.TABLE if c.id != "big"]
    assert all(c.ntraj == 8 and 2 <= c.L <= 5 for c in T.TABLE)
    assert all(c.C % 2 == 1 and 9 <= c.C <= 31 for c in small if c.D < 257 and c.id[0] in "rwm" and "c" not in c.id)
    assert all(5 <= c.C <= 9 and c.C % 2 == 1 for c in T.TABLE if c.D >= 257)
    by = lambda routes: {c.D for c in T.TABLE if set(routes) <= set(c.routes) and c.mass == "none" and c.burn == T.BURN}
    assert by(T.SMALL32) >= {1, 2, 3, 4, 5, 6} and by(T.SMALL64) >= {1, 3, 4}
    assert by(T.WAVE32) >= {7, 63, 64, 65, 127, 128, 129} and by(T.WAVE64) >= {5, 6, 99, 100}
    assert by(("wave",)) >= {64, 65, 128, 129, 256, 257, 512, 513, 1024}
    assert {c.D for c in T.TABLE if c.mass == "full" and "wave" in c.routes} >= {7, 65, 257}
    assert {(c.D, c.mass) for c in T.TABLE if set(T.SMALL32) <= set(c.routes)} >= {(d, m) for d in (3, 6) for m in ("none", "diag", "full")}
    assert {c.burn for c in T.TABLE if c.D == 3 and c.mass == "none" and c.C == 31} == {-1, 0, 2, T.NTRAJ - 1} == {c.burn for c in T.TABLE if c.D == 7 and c.C == 31}
    assert {c.C % 4 for c in T.TABLE if c.D == 7 and c.mass == "none" and c.burn == T.BURN and c.C < 100} == {0, 1, 2, 3}
    assert C["big"].C > 4 * 65535 and (C["big"].C + 3) // 4 > 65535 and T.probe_chains(C["big"]).size == 17
    sel = T.probe_chains(C["big"])
    assert list(sel[:4]) == [0, 1, 2, 3] and list(sel[-4:]) == list(range(T.BIG_C - 4, T.BIG_C)) and np.all(np.diff(sel) > 0)
    assert [C[k].C for k in ("e63", "e64", "e65")] == [63, 64, 65] and [C[k].C for k in ("q15", "q16", "q17")] == [15, 16, 17]
    assert all(C[k].C in (24, 40) for k in ("qo1", "qo2", "qo3", "qo4")) and "small_cpb" in C["e65"].routes
    assert set(T.CUT_IDS) <= set(C) and set(T.PAD_IDS) <= set(C) and all(C[k].burn == T.BURN for k in T.CUT_IDS)
    assert set(T.STEPS) == set(C) == set(T.H_DIST)
    assert all(c.f in T.F_GRID and T.SEED_BASE <= c.seed < T.SEED_BASE + 3 for c in T.TABLE)


def test_the_restated_launcher_sends_every_case_where_it_claims():
    """Every kernel of hmc_gaussian.hip reachable through hta_hmc_gaussian_sample is reached with its per-trajectory outputs at every D,
    R, dtype and mass kind listed below, and without them (the instances a plain sample() launches) at the sizes listed below - not at
    every D; a refusal lands where it is named."""
    C = T.CASES
    seen = {T.expected_route(C[cid], r) for cid, r in T.runs()}
    for Tn, dims in (("float", (1, 2, 3, 4, 5, 6)), ("double", (1, 3, 4))):
        for D in dims:
            assert "hmc_gauss_small_kernel<%s,%d,0,true,true>" % (Tn, D) in seen and "hmc_gauss_small_kernel<%s,%d,0,false,true>" % (Tn, D) in seen
            assert "hmc_gauss_eig_kernel<%s,%d,true>" % (Tn, D) in seen
    for D in (3, 6):
        for kind in (1, 2):
            assert "hmc_gauss_small_kernel<float,%d,%d,true,true>" % (D, kind) in seen and "hmc_gauss_small_kernel<float,%d,%d,false,true>" % (D, kind) in seen
    assert "hmc_gauss_eig_kernel<float,3,false>" in seen and "hmc_gauss_eig_kernel<float,5,false>" in seen
    # the instances without the per-trajectory outputs (what a plain sample() launches): each form once at D = 3, and with a dense mass
    assert {"hmc_gauss_small_kernel<float,3,0,false,false>", "hmc_gauss_small_kernel<float,3,0,true,false>", "hmc_gauss_small_kernel<double,3,0,false,false>",
            "hmc_gauss_small_kernel<float,6,0,false,false>", "hmc_gauss_small_kernel<float,6,0,true,false>", "hmc_gauss_small_kernel<float,3,2,false,false>",
            "hmc_gauss_small_kernel<double,3,2,false,false>", "hmc_gauss_eig_kernel<double,3,false>"} <= seen
    for D in (1, 2, 3, 4):
        assert "hmc_gauss_quad_kernel<%d,true,0>" % D in seen
        assert any(s.startswith("hmc_gauss_quad_kernel<%d,false," % D) and s.endswith(",7>") for s in seen)
        assert any(s.startswith("hmc_gauss_quad_fused_kernel<%d," % D) for s in seen)
    assert {"hmc_gauss_quad_kernel<4,false,5,7>", "hmc_gauss_quad_kernel<3,false,0,7>", "hmc_gauss_quad_fused_kernel<2,5>", "hmc_gauss_quad_fused_kernel<3,0>"} <= seen
    for R in (1, 2, 4, 8, 16):
        for kind in (0, 1, 2):
            assert "hmc_gauss_wave_kernel<float,%d,%d>" % (R, kind) in seen, (R, kind)
    assert {"hmc_gauss_wave_kernel<double,1,0>", "hmc_gauss_wave_kernel<double,2,0>", "hmc_gauss_wave_kernel<double,1,2>"} <= seen
    assert {"hmc_gauss_wave_eig_kernel<%s,%d>" % (Tn, R) for Tn in ("float", "double") for R in (1, 2)} <= seen
    # the routes by name
    assert T.expected_route(C["r3"], "small_inline") == "hmc_gauss_small_kernel<float,3,0,false,true>"
    assert T.expected_route(C["r3f"], "small_ws") == "hmc_gauss_small_kernel<float,3,2,true,true>"
    assert T.expected_route(C["r3"], "eig") == "hmc_gauss_eig_kernel<float,3,true>" == T.expected_route(C["r3"], "eig_cap")
    assert T.expected_route(C["r3d"], "quad_diag") == "hmc_gauss_quad_kernel<3,true,0>"
    assert T.expected_route(C["r4"], "quad_two") == "hmc_gauss_quad_kernel<4,false,5,7>"
    assert T.expected_route(C["r3"], "general_small") == "hmc_gauss_wave_kernel<float,1,0>" and T.expected_route(C["r6f"], "general_small") == "hmc_gauss_wave_kernel<float,1,2>"
    assert T.expected_route(C["r4"], "eig_f64") == "hmc_gauss_eig_kernel<double,4,true>"
    assert T.expected_route(C["r5"], "wave_eig_f64") == "hmc_gauss_wave_eig_kernel<double,1>" and T.expected_route(C["r5"], "wave_f64") == "hmc_gauss_wave_kernel<double,1,0>"
    assert T.expected_route(C["w64"], "wave") == "hmc_gauss_wave_kernel<float,1,0>" and T.expected_route(C["w65"], "wave") == "hmc_gauss_wave_kernel<float,2,0>"
    assert T.expected_route(C["w128"], "wave_eig") == "hmc_gauss_wave_eig_kernel<float,2>" and T.expected_route(C["w64"], "wave_eig") == "hmc_gauss_wave_eig_kernel<float,1>"
    assert [T.wave_r(D) for D in (7, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    # the refusals by name: D = 129 off the eigenbasis route, a dense (or any) mass off wave_eig, D = 5 off the quad route, C % 8 != 0 off quad_one
    assert T.expected_route(C["w129"], "wave_eig") == "hmc_gauss_wave_kernel<float,4,0>"
    assert T.expected_route(C["m7f"], "wave_eig") == "hmc_gauss_wave_kernel<float,1,2>" and T.expected_route(C["m65f"], "wave_eig") == "hmc_gauss_wave_kernel<float,2,2>"
    assert T.expected_route(C["m64d"], "wave_eig") == "hmc_gauss_wave_kernel<float,1,1>"
    assert T.expected_route(C["r5"], "quad_diag") == "hmc_gauss_eig_kernel<float,5,true>" and T.expected_route(C["r5"], "quad_two") == "hmc_gauss_eig_kernel<float,5,false>"
    assert T.expected_route(C["q15"], "quad_one") == T.expected_route(C["q17"], "quad_one") == "hmc_gauss_quad_kernel<3,false,0,7>"
    assert T.expected_route(C["q16"], "quad_one") == "hmc_gauss_quad_fused_kernel<3,0>" == T.expected_route(C["qo3"], "quad_one")
    # a launch of fewer than 8 trajectories, or of another count than the workspace was prepared for, leaves the one-launch route
    assert T.expected_route(C["qo3"], "quad_one", 5) == "hmc_gauss_quad_kernel<3,false,0,7>" == T.expected_route(C["qo3"], "quad_two", 3)
    assert T.carries_only_the_point(T.expected_route(C["w7"], "wave")) and not T.carries_only_the_point(T.expected_route(C["w7"], "wave_eig"))


def test_the_workspace_formula():
    # D <= 6: (n_traj + 4 rows of look-ahead) records of D + 1 values padded to 16 bytes, then the 128-element eig block
    assert T.workspace_bytes(31, 3, 8, 4) == 12 * 31 * 16 + 512
    assert T.workspace_bytes(19, 4, 8, 4) == 12 * 19 * 32 + 512
    assert T.workspace_bytes(31, 3, 8, 8) == 12 * 31 * 32 + 1024
    assert T.workspace_bytes(17, 5, 8, 8) == 12 * 17 * 48 + 1024
    assert T.workspace_bytes(24, 1, 8, 4) == 12 * 24 * 16 + 512
    # D > 6: V | Vt | lam + 64 elements, rounded to 16 bytes; the chain count does not enter
    assert T.workspace_bytes(31, 7, 8, 4) == (2 * 49 + 7 + 64) * 4 + 12 == T.workspace_bytes(5, 7, 99, 4)
    assert T.workspace_bytes(9, 129, 8, 4) == (2 * 129 * 129 + 129 + 64) * 4 + 4
    assert T.workspace_bytes(9, 99, 8, 8) == (2 * 99 * 99 + 99 + 64) * 8 + 8
    # float64 from D = 100: the slab of the diagonalisation, both matrices (D x D and D x (D + 1) at an even D) behind the eig area
    assert T.metric_slab_bytes(99, 8) == 0 and T.metric_slab_bytes(100, 8) == (100 * 100 + 100 * 101) * 8 and T.metric_slab_bytes(128, 4) == 0
    assert T.workspace_bytes(9, 100, 8, 8) == (2 * 100 * 100 + 100 + 64) * 8 + 160800
    assert T.workspace_bytes(9, 1024, 8, 4) == (2 * 1024 * 1024 + 1024 + 64) * 4


def test_the_inputs_are_the_ones_described():
    for D in sorted({c.D for c in T.TABLE}):
        P, mu = T.inputs_of(D)
        lam = np.linalg.eigvalsh(P.astype(np.float64))
        assert P.dtype == mu.dtype == np.float32 and np.array_equal(P, P.T) and abs(lam.min() - 0.5) < 1e-5 and abs(lam.max() - (2.0 if D > 1 else 0.5)) < 1e-5
        assert np.array_equal(mu, np.linspace(-1, 1, D).astype(np.float32)) and np.abs(mu).max() == 1.0 and T.log_norm(D) != 0.0
    for c in T.TABLE:
        if c.id == "big":
            continue
        th0 = T.starts(c)
        mu = T.inputs_of(c.D)[1]
        assert th0.dtype == np.float32 and th0.shape == (c.C, c.D) and 0.05 < np.abs(th0 - mu).std() / 0.3 < 2.0
        assert np.array_equal(T.starts(c, [c.C - 1])[0], th0[-1])
        kind, im, mf = T.mass_operands(c, np.float32)
        assert kind == T.MASS_KIND[c.mass]
        if kind == 1:
            assert im.shape == mf.shape == (c.D,) and 0.5 <= im.min() and im.max() <= 2.0 and np.allclose(mf * mf * im, 1.0, atol=1e-6)
        if kind == 2:
            lam = np.linalg.eigvalsh(im.astype(np.float64))
            assert np.array_equal(im, im.T) and abs(lam.min() - 0.5) < 1e-5 and abs(lam.max() - 1.5) < 1e-5
            assert np.array_equal(mf, np.tril(mf)) and np.allclose(mf.astype(np.float64) @ mf.T @ im, np.eye(c.D), atol=1e-5)
            assert np.abs(np.tril(mf, -1)).max() > 0.01          # a factor whose strict lower triangle and diagonal both matter
        # the step size is inside the stability limit and in the search's grid
        assert 0.0 < T.eps_of(c) < 2.0 / T.omega_max(c.D, c.mass)


@pytest.mark.parametrize("cid", [c.id for c in T.TABLE])
def test_every_case_discriminates(cid):
    """The float64 oracle alone: acceptance over chains x trajectories in [0.2, 0.9]; at trajectory burn + 1 at least one chain accepts
    and one rejects, and a rejecting one had moved more than 100 row bands from theta_init (where burn + 1 exists; at burn = -1 the
    reset row is the start itself); the run with the mean at 0, with log_norm at 0 and without the mass operand each move an energy of
    trajectory 0 beyond its tolerance; on the two-launch cases the draws restarted at the cut would be noticed; the oracle entirely in
    float32 stays within a third of every float32 bound and flips no decision; on a case with a float64 route no decision lies within
    GUARD max(1, |H|) of its threshold.  The recorded float32 distance of the energies is the measured one, rounded up."""
    case = T.CASES[cid]
    ref = discriminates(case)
    assert ref.rows.shape == (case.ntraj - case.burn, T.probe_chains(case).size, case.D)
    d = T.h_distance(case)
    assert d <= T.H_DIST[cid] <= max(1.25 * d, d + 1e-12), (d, T.H_DIST[cid])


@pytest.mark.parametrize("cid", ["r3", "m7f"])
def test_the_recorded_steps_are_what_the_search_finds(cid):
    """The deterministic search over F_GRID x three seeds, run again on two cheap cases: the recorded (f, seed, tried)."""
    assert T.search(cid, lambda c: discriminates(c, report=lambda *_: None)) == T.STEPS[cid]
    assert T.max_outside("f32", 17) == 0 and T.max_outside("f32", 31) == 1 and T.max_outside("f32", 65) == 3 and T.max_outside("f64", 31) == 0


if __name__ == "__main__":
    quiet = lambda *_: None
    ids = sys.argv[1:] or [c.id for c in T.TABLE]
    steps, dists = {}, {}
    for cid in ids:
        f, seed, tried = T.search(cid, lambda c: discriminates(c, report=quiet))
        steps[cid] = (f, seed, tried)
        dists[cid] = _round_up(T.h_distance(T.CASES[cid]._replace(f=f, seed=seed)))
        print("    %r: %r," % (cid, steps[cid]), "   # H_DIST %r: %r," % (cid, dists[cid]), flush=True)
    print("STEPS = {\n" + "".join("    %r: %r,\n" % kv for kv in steps.items()) + "}")
    print("H_DIST = {\n" + "".join("    %r: %r,\n" % kv for kv in dists.items()) + "}")
