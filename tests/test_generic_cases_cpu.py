"""No GPU: everything tests/test_gpu_pieces.py and tests/test_gpu_generic.py take for granted about tests/generic_cases.py - the numpy
twins against torch.autograd, the recorded float32 distances measured again, the float32 oracle against the float64 oracle on every
float32 engine run (no flipped chain, both Metropolis branches at trajectory burn + 1), the oracle's rates the carry and divergence
tests ask for, and the guard band of the Metropolis-select cases."""
import numpy as np
import pytest
import torch

import generic_cases as G

f64 = torch.float64


# ---- targets ----------------------------------------------------------------------------------------------------------------------------
TWINS = {"gauss1": G.DenseGaussian(1), "gauss5": G.DenseGaussian(5), "gauss130": G.DenseGaussian(130), "funnel": G.Funnel(11),
         "ball": G.Ball(4, 2.5), "branching": G.Branching(4), "split_subset": G.DenseGaussian(65, 2)}


@pytest.mark.parametrize("name", sorted(TWINS))
def test_the_numpy_twins_against_autograd(name):
    """log p and gradient of every twin, batched, against torch.autograd of its own closure in float64 at a dozen points: 1e-10 relative
    to 1 + |ref|.  The ball's points lie on both sides of its radius (NaN outside, gradient 0), the branching callable's on both sides
    of its `if`.  A float32 argument is evaluated in float32."""
    tgt = TWINS[name]
    fn = tgt.closure(f64, "cpu")
    pts = (1.6 if name == "ball" else 0.7) * np.random.default_rng(7).standard_normal((12, tgt.D))
    mine = np.concatenate([tgt.logp(pts)[:, None], tgt.grad(pts)], 1)
    assert mine.shape == (12, 1 + tgt.D) and mine.dtype == np.float64
    if name == "ball":
        assert 2 <= np.isnan(mine[:, 0]).sum() <= 10
    if name == "branching":
        assert 2 <= (pts[:, 0] < 0).sum() <= 10
    for k in range(12):
        x = torch.tensor(pts[k], dtype=f64, requires_grad=True)
        v = fn(x)
        g, = torch.autograd.grad(v, x)
        ref = np.concatenate([[float(v.detach())], g.numpy()])
        assert np.array_equal(np.isnan(mine[k]), np.isnan(ref))
        ok = ~np.isnan(ref)
        assert np.all(np.abs(mine[k] - ref)[ok] <= 1e-10 * (1.0 + np.abs(ref[ok]))), (k, mine[k], ref)
    low = pts.astype(np.float32)
    assert tgt.logp(low).dtype == np.float32 and tgt.grad(low).dtype == np.float32


def test_the_gradient_handed_in_is_not_the_callables_own():
    """pass_grad: the oracle integrates the gradient of ANOTHER Gaussian (and a constant vector), so an engine that ignored
    `pass_grad` and differentiated the callable would not reproduce it."""
    pts = np.random.default_rng(3).standard_normal((4, 5))
    for name in ("pass_grad_callable", "pass_grad_tensor"):
        t = G.RUNS[name].target
        assert np.abs(t.grad(pts) - t.logp_of.grad(pts)).min() > 1e-3
    g = G.PASS_GRAD_OTHER.grad_closure(f64, "cpu")(torch.tensor(pts[0]))
    assert np.allclose(g.numpy(), G.PASS_GRAD_OTHER.grad(pts[:1])[0], atol=1e-12)


def test_the_non_symmetric_matrix_tells_the_two_index_orders_apart():
    for D in (2, 17, 130):
        A, x = G.inv_mass("nonsym", D), G.piece_inputs(D)["p"]
        assert np.abs(G.matvec(x, A) - G.matvec(x, A.T)).max() > 0.1
        assert np.allclose(G.matvec(x, A), x @ A.T, atol=1e-12)                 # the oracle's _apply_inv_mass
        S = G.inv_mass("full", D)
        assert np.array_equal(S, S.T) and np.linalg.eigvalsh(S).min() > 0.4


# ---- kernel-level float32 bounds ---------------------------------------------------------------------------------------------------------
def test_every_kernel_level_case_has_a_bound():
    assert sorted(G.F32_PIECES) == sorted(G.piece_cases())


@pytest.mark.parametrize("case", [c for c in G.piece_cases() if c[3] == 70 or c[1] != "full"], ids=lambda c: "-".join(map(str, c)))
def test_the_recorded_float32_distances(case):
    """F32_PIECES is what f32_distance measures (rounded up to two digits when it was recorded): not below the measurement, not above
    twice it - nobody widened it by hand; the scale to 1 %.  (The full-mass grid-stride rows are measured by the test below.)"""
    dist, scale = G.f32_distance(*case)
    rec, rec_scale = G.F32_PIECES[case]
    print(case, "measured %.3g recorded %.3g scale %.3g" % (dist, rec, scale))
    assert dist <= rec <= max(2.0 * dist, 1e-12)
    assert abs(scale - rec_scale) <= 0.01 * scale


def test_the_recorded_float32_distances_of_the_large_full_mass_rows():
    for case in [c for c in G.piece_cases() if c[3] != 70 and c[1] == "full"]:
        dist, scale = G.f32_distance(*case)
        rec, rec_scale = G.F32_PIECES[case]
        assert dist <= rec <= 2.0 * dist and abs(scale - rec_scale) <= 0.01 * scale, (case, dist, scale)


def test_the_recorded_float32_distances_of_the_leapfrog_paths():
    for (D, mass), (rec, rec_scale) in G.F32_LEAPFROG.items():
        a, b = G.leapfrog_path(D, mass, np.float32, np.float32), G.leapfrog_path(D, mass, np.float32, np.float64)
        assert a[0].dtype == np.float32 and b[0].dtype == np.float64 and a[0].shape == (G.LEAPFROG[D][0], D)
        dist = max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())
        scale = max(np.abs(b[0]).max(), np.abs(b[1]).max())
        assert dist <= rec <= 2.0 * dist and abs(scale - rec_scale) <= 0.01 * scale, (D, mass, dist, scale)
    assert sorted(G.F32_LEAPFROG) == sorted((D, m) for D in G.LEAPFROG for m in G.MASSES)


def test_the_float32_box_muller_is_the_oracles_stream():
    a = G.normals32(G.RS_SEED, G.RS_OFF + np.arange(9), G.RS_DRAW, 130)
    b = G.O.philox_normals(G.RS_SEED, G.RS_OFF + np.arange(9), G.RS_DRAW, 130, dtype=np.float64)
    assert a.dtype == np.float32 and a.shape == b.shape and 0 < np.abs(a - b).max() < 5e-6


# ---- Metropolis select -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_no_chain_of_the_select_cases_lies_in_the_guard_band(dt):
    """Every random-class chain is at least MH_GUARD (1 + |H_old| + |H_new|) from its threshold at the four trajectory indices, so
    the decisions are compared exactly with NO chain left out; every class decides as it is named, the random class both ways."""
    Ho, Hn, lp, klass = G.mh_inputs(70, dt)
    assert sorted(np.flatnonzero(klass == "n")) == sorted(G.NONFINITE) and (klass == "x").sum() >= 40
    for n in G.MH_N:
        u = G.mh_uniform(n, 70, dt)
        assert u.dtype == dt and (G.mh_margin(Ho, Hn, u)[klass == "x"] >= G.MH_GUARD).all()
        for with_lp in (True, False):
            acc = G.mh_expected(np.zeros((70, 1)), np.ones((70, 1)), np.zeros((70, 1)), Ho, Hn, lp if with_lp else None, n, G.MH_BURN, u,
                                np.zeros(70, np.int64))[0]
            assert acc[klass == "a"].all() and not acc[klass == "r"].any()
            assert 5 <= acc[klass == "x"].sum() <= (klass == "x").sum() - 5
            for c, (which, _) in G.NONFINITE.items():
                assert acc[c] == (which == "lp" and not with_lp), (c, which)         # without log p the energies alone decide


def test_the_select_rule_is_the_drivers():
    """mh_expected applied trajectory by trajectory reproduces O.sample_chain_driver (rows, current state and reject counts)."""
    rng = np.random.default_rng(1)
    C, D, N, burn = 6, 2, 7, 2
    init = rng.standard_normal((C, D))
    props = rng.standard_normal((N, C, D))
    accs = rng.uniform(size=(N, C)) < 0.5
    accs[burn + 1, :2] = False
    ret, rej = G.O.sample_chain_driver(C, D, np.float64, init, N, burn, lambda n, cur: (props[n], accs[n]))
    cur, rows, count = init.copy(), [init.copy()], np.zeros(C, np.int64)
    for n in range(N):
        Ho = np.zeros(C)
        Hn = np.where(accs[n], -1.0, 100.0)          # sure accept / sure reject
        acc, cur, row, count = G.mh_expected(cur, props[n], init, Ho, Hn, None, n, burn, np.full(C, 0.5), count)
        assert np.array_equal(acc, accs[n])
        if row is not None:
            rows.append(row)
    assert np.array_equal(np.stack(rows), np.stack(ret)) and np.array_equal(count, rej)


# ---- engine runs --------------------------------------------------------------------------------------------------------------------------
def flipped_and_deviation(run):
    (a, ia), (b, ib) = run.oracle(torch.float32), run.oracle(torch.float32, exact=True)
    flipped = (np.stack(ia["accept"]) != np.stack(ib["accept"])).any(0)
    return flipped, G.deviation(a, b), ia


def test_every_float32_run_has_a_recorded_error():
    assert sorted(G.F32_ORACLE_ERR) == sorted(G.F32_RUNS)


@pytest.mark.parametrize("name", G.F32_RUNS)
def test_the_float32_oracle_on_every_float32_run(name):
    """The two conditions the GPU tests rely on: the float32 oracle flips NO chain against the float64 oracle on the same draws (the
    3 % exempt share is then the kernels' alone), and its largest difference is what F32_ORACLE_ERR records (not above it, not below
    half of it).  Both Metropolis branches are taken at trajectory burn + 1: some chains accept, some reject and restart from
    params_init."""
    run = G.RUNS[name]
    flipped, err, info = flipped_and_deviation(run)
    q2 = np.stack(info["accept"])[run.burn + 1]
    print("%s: %d flipped, largest difference %.3g (recorded %.3g, bound %.3g), acceptance %.2f, %d of %d reject at burn + 1"
          % (name, flipped.sum(), err.max(), G.F32_ORACLE_ERR[name], run.bound(torch.float32), info["acc_rate"].mean(), (~q2).sum(), q2.size))
    assert flipped.sum() == 0
    assert err.max() <= G.F32_ORACLE_ERR[name] <= 2.0 * err.max()
    assert 0 < (~q2).sum() < q2.size
    assert run.bound(torch.float32) == (G.BAND_F32 if run.band else max(4.0 * G.F32_ORACLE_ERR[name], 2e-6))
    assert run.band == name.startswith("funnel")
    q2_64 = np.stack(run.oracle(f64)[1]["accept"])[run.burn + 1]
    assert 0 < (~q2_64).sum() < q2_64.size


def test_the_engine_table_is_the_issues():
    """Dense Gaussians at D = 1, 5, 11, 65, 130 and the 11-D funnel, 70 chains, 12 trajectories of at most 8 steps, seed 4242, chain
    offset 17, the three (mass, burn) rows."""
    assert len(G.ORACLE_RUNS) == 18 and G.MASS_ROWS == (("none", 0), ("diag", 3), ("full", -1))
    for name in G.ORACLE_RUNS:
        r = G.RUNS[name]
        assert (r.C, r.N, r.seed, r.off) == (70, 12, 4242, 17) and r.L <= 8 and (r.mass, r.burn) in G.MASS_ROWS
        assert r.scale == (0.5 if r.band else 0.3)
    assert sorted({G.RUNS[n].D for n in G.ORACLE_RUNS if not G.RUNS[n].band}) == [1, 5, 11, 65, 130]


@pytest.mark.parametrize("dtype", [torch.float32, f64], ids=["f32", "f64"])
def test_the_carry_run_rejects_between_30_and_70_percent(dtype):
    info = G.RUNS["carry"].oracle(dtype)[1]
    assert 0.3 <= 1.0 - info["acc_rate"].mean() <= 0.7
    acc = np.stack(info["accept"])
    assert (acc.any(0) & (~acc).any(0)).mean() >= 0.9          # nearly every chain uses the carried pair on both branches


def test_the_ball_run_diverges_and_moves():
    """float64, the oracle: at least 5 non-finite proposals, and finite accepted ones in EVERY chain - the threshold of 5 divided by
    the 70 columns is less than one accept, taken from the column with the fewest, not from a mean.  No chain starts outside."""
    run = G.RUNS["ball"]
    ref, info = run.oracle(f64)
    hn, acc = np.stack(info["h_new"]), np.stack(info["accept"])
    assert np.isfinite(np.stack(info["h_old"])).all() and np.isfinite(ref).all()
    assert (~np.isfinite(hn)).sum() >= 5 and not acc[~np.isfinite(hn)].any()
    assert (np.isfinite(hn) & acc).sum(0).min() >= 5.0 / run.C
    assert (~np.isfinite(hn)).any(0).sum() >= 35 and not (~np.isfinite(hn)).all(0).any()


def test_the_loop_run_takes_both_sides_of_the_branch():
    ref, info = G.RUNS["loop"].oracle(f64)
    assert (ref[..., 0] < 0).any() and (ref[..., 0] > 0).any() and 0.3 <= info["acc_rate"].mean() < 1.0
