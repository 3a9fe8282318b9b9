"""No GPU: everything tests/test_gpu_mlp_traj.py takes for granted about tests/mlp_traj_cases.py, checked on the oracle alone - the
table is the one asked for, the fast target is the oracle's MLPRegressionTarget, and every case can tell a wrong kernel from a right
one: it rejects and accepts, the Q2 reset at trajectory burn + 1 runs and is told apart from "keep current", the float32 arithmetic
does not move a chain across a ReLU kink or a Metropolis threshold, a float64 decision has room, and the diagonal mass matters."""
import numpy as np
import pytest

import hmc_oracle as O
import mlp_traj_cases as T


def _report(name, case, ref):
    q2 = ref.accept[T.BURN + 1]
    print("%s: eps %g, acceptance %.2f, %d of %d chains reject at burn + 1" % (name, case.eps, ref.accept.mean(), (~q2).sum(), q2.size))
    return q2


def test_the_table_is_the_one_asked_for():
    """32 chains, L = 3, 7 trajectories, burn 1, tau = [1, 1.5, 2, 2.5]; the shapes, integrators and masses per id; which ids run
    on which route; the instance every (route, id) must report."""
    assert (T.C, T.L, T.NTRAJ, T.BURN, T.TAU) == (32, 3, 7, 1, (1.0, 1.5, 2.0, 2.5))
    want = {"m1": (4, 17, "tanh", 24, 3, "symmetric", "diag"), "m2": (5, 48, "relu", 40, 2, "kmid", "diag"),
            "m3": (12, 40, "sigmoid", 72, 2, "rand", "none"), "m4": (16, 33, "relu", 150, 2, "symmetric", "diag"),
            "m5": (9, 130, "tanh", 36, 2, "symmetric", "diag"), "m6": (2, 16, "relu", 50, 1, "leapfrog", "diag"),
            "m7": (8, 100, "relu", 100, 4, "symmetric", "diag"), "m8": (1, 256, "tanh", 16, 2, "rand", "diag"),
            "m9": (4, 17, "tanh", 24, 3, "symmetric", "diag"), "v1": (4, 65, "tanh", 24, 3, "symmetric", "diag"),
            "v2": (17, 600, "relu", 20, 2, "symmetric", "diag"), "v3": (32, 130, "sigmoid", 36, 2, "kmid", "diag"),
            "v4": (8, 300, "relu", 300, 2, "rand", "none")}
    assert {k: tuple(c[1:8]) for k, c in T.CASES.items()} == want
    for c in T.CASES.values():
        assert (c.C, c.L, c.ntraj) == (32, 3, 7) and c.tau_out == (100.0 if c.id == "m7" else 6.0)
        assert c.extra_rows == (5 if c.id == "m9" else 0)
    assert T.MFMA_IDS == ("m1", "m2", "m3", "m4", "m5", "m6", "m7", "m8") and T.VALU_IDS == ("m1", "m4", "m6", "v1", "v2", "v3", "v4")
    assert T.F64_IDS == ("m1", "m4", "v1", "v3") and len(T.RUNS) == 19
    for route, cid in T.RUNS + [("mfma", "m9")]:
        c, name = T.CASES[cid], T.expected_route(route, cid)
        if route == "mfma":          # <NK, NPT, ACT, NTMAX>: csrc/mlp_mfma.hip's dispatch, restated
            npt = 8 if c.H > 128 else min(8, (c.Nb + 15) // 16)
            assert name == "mlp_mfma_kernel<%d,%d,%d,%d>" % ((c.n_in + 3) // 4, npt, T.ACT_ID[c.act], 1024 if c.H > 128 else 512)
        else:                        # <T, INMAX, NT, ACT, EXACT>: csrc/mlp_hmc.hip's
            inmax = next(w for w in (4, 8, 16, 32) if c.n_in <= w)
            assert name == "mlp1_hmc_kernel<%s,%d,%d,%d,%s>" % ("double" if route == "f64" else "float", inmax, 512 if c.H <= 512 else 1024,
                                                                T.ACT_ID[c.act], "true" if c.n_in == inmax else "false")
    g = T.GRID_CASES
    assert (g["mfma"].C, g["valu"].C) == (8193, 4097)
    for c in g.values():
        assert tuple(c[1:8]) == (1, 3, "relu", 4, 2, "symmetric", "diag") and (c.L, c.ntraj) == (2, 4)
    # the edges the shapes were chosen for (csrc/mlp_hmc.hip:launch_mlp_act): unit groups UG, point slices PS, idle waves, chunks
    for cid, ug, ps, idle in [("v1", 2, 4, 0), ("v2", 10, 1, 6), ("v3", 3, 2, 2), ("v4", 5, 1, 3)]:
        c = T.CASES[cid]
        waves = (512 if c.H <= 512 else 1024) // 64
        assert ((c.H + 63) // 64, waves // ((c.H + 63) // 64), waves - ug * ps) == (ug, ps, idle)
    assert T.CASES["v4"].Nb > 256 and T.CASES["m4"].Nb > 128 and T.CASES["m2"].H % 16 == 0


@pytest.mark.parametrize("cid", sorted(T.ALL_CASES))
def test_the_fast_target_is_the_oracles(cid):
    """Value and gradient of every split's target against oracle/hmc_oracle.py:MLPRegressionTarget itself at four starting points,
    float64: 1e-12 relative to the largest entry; the value-only path gives the same value."""
    case = T.ALL_CASES[cid]
    th = T.inputs(cid)[2][:4].astype(np.float64)
    for mine, ref in zip(T.targets(case), T.targets(case, O.MLPRegressionTarget)):
        assert isinstance(mine, O.MLPRegressionTarget) and type(ref) is O.MLPRegressionTarget
        (a, ga), (b, gb) = mine.logp_and_grad(th), ref.logp_and_grad(th)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max() and np.abs(ga - gb).max() <= 1e-12 * np.abs(gb).max()
        assert np.array_equal(mine.logp(th), a) and np.array_equal(mine.grad(th), ga)


def test_the_unused_rows_are_behind_the_splits():
    """m9 is m1 with five rows of 1e6 appended: the same inputs otherwise, so the same oracle, and rows a kernel must never read
    as data (one of them in the full-data pass would move log p by 1e12)."""
    a, b = T.inputs("m1"), T.inputs("m9")
    assert b[0].shape[0] == a[0].shape[0] + 5 and (b[0][-5:] == 1e6).all() and (b[1][-5:] == 1e6).all()
    assert np.array_equal(b[0][:-5], a[0]) and np.array_equal(b[1][:-5], a[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert np.array_equal(T.reference("m9").samples, T.reference("m1").samples)


@pytest.mark.parametrize("cid", sorted(T.CASES))
def test_every_case_discriminates(cid):
    """The float64 oracle alone: acceptance over all chains and trajectories in [0.2, 0.9]; at trajectory burn + 1 at least 2 chains
    reject (their row is params_init again) and at least 2 accept; the float32-state oracle is further than 5e-4 from the float64
    one on at most 1 of the 32 chains (a ReLU kink or a threshold crossed by rounding alone); in a float64 case no decision lies
    within GUARD max(1, |H|) of its threshold.  A chain that rejected at burn + 1 moved before (or its reset could not be told
    from keeping the current point)."""
    case, ref = T.CASES[cid], T.reference(cid)
    q2 = _report(cid, case, ref)
    assert ref.samples.shape == (T.n_rows(case), case.C, T.n_params(case)) and np.isfinite(ref.samples).all()
    assert 0.2 <= ref.accept.mean() <= 0.9
    assert (~q2).sum() >= 2 and q2.sum() >= 2
    assert np.array_equal(ref.samples[1][:, :][~q2], T.inputs(cid)[2][~q2].astype(np.float64))
    moved = ref.accept[:T.BURN + 1].any(0)
    assert (moved & ~q2).sum() >= 2          # accepted during burn-in, rejected at burn + 1: "keep current" would give another row
    low = T.run_oracle(case, dtype=np.float32)
    assert low.samples.dtype == np.float32
    far = T.outside(low.samples.astype(np.float64), ref.samples, T.KINK_TOL)
    margin = T.guard_margin(ref)
    print("%s: float32 oracle further than %g on %d chains (largest %.3g); closest decision %.3g max(1, |H|), |H| up to %.4g"
          % (cid, T.KINK_TOL, far.sum(), np.abs(low.samples - ref.samples).max(), margin.min(), np.abs(ref.h_old).max()))
    assert far.sum() <= T.KINK_MAX_CHAINS
    assert np.isfinite(ref.h_old).all() and np.isfinite(ref.h_new[0]).all()
    if cid in T.F64_IDS:
        assert margin.min() >= T.GUARD
    assert np.array_equal(ref.rejected, (~ref.accept).sum(0)) and ref.rejected.max() > ref.rejected.min()


class _ScaledDraws(O.PhiloxDraws):
    """The oracle derives the momentum factor from the inverse mass it is given; a kernel loads the two from separate vectors.
    Scaling the normals by sqrt(wrong / right) gives the oracle the momenta of the RIGHT factor beside a WRONG inverse mass."""

    def __init__(self, seed, ids, scale):
        super().__init__(seed, ids, dtype=np.float64)
        self.scale = scale

    def normals(self, n, D, sub=0):
        return super().normals(n, D, sub) * self.scale


@pytest.mark.parametrize("cid", [c for c in sorted(T.CASES) if T.CASES[c].mass == "diag"])
def test_the_diagonal_mass_matters(cid):
    """What a wrong mass offset would do to the GPU test.  The oracle run again as a kernel would compute that reads the inverse
    mass of the b1 block from the W2 block's offsets - in M^-1 alone (kinetic energy and drift; the draw keeps the right factor)
    and in both vectors: either an energy of trajectory 0 leaves the float32 tolerance (the GPU test exempts no chain there) or
    more than twice the 7 % of the chains the sample band exempts leave it."""
    case, ref = T.CASES[cid], T.reference(cid)
    X, Y, th0, im = T.inputs(cid)
    tol = T.ENERGY_TOL["f32"] * max(1.0, np.abs(ref.h_old[0]).max(), np.abs(ref.h_new[0]).max())
    o_b1, H = case.H * case.n_in, case.H
    shifted = im.astype(np.float64)
    shifted[o_b1:o_b1 + H] = im[o_b1 + H:o_b1 + 2 * H]
    assert np.abs(shifted - im).max() > 0.1
    ids = T.CHAIN_OFFSET + np.arange(case.C)
    for what, scale in (("M^-1 of b1 from W2", np.sqrt(shifted / im)), ("M^-1 and sqrt(M) of b1 from W2", 1.0)):
        tg = T.targets(case)
        draws = _ScaledDraws(case.seed, ids, scale)
        start = th0.astype(np.float64)
        if case.integ == "leapfrog":
            ret, info = O.sample_hmc(tg[0], start, case.ntraj, case.L, case.eps, T.BURN, shifted, draws)
        else:
            ret, info = O.sample_hmc(None, start, case.ntraj, case.L, case.eps, T.BURN, shifted, draws, grad_fns=[t.grad for t in tg],
                                     logp_fns=[t.logp for t in tg], split_kind=case.integ)
        d_old, d_new = np.abs(info["h_old"][0] - ref.h_old[0]), np.abs(info["h_new"][0] - ref.h_new[0])
        out = T.outside(np.stack(ret), ref.samples, T.SAMPLE_TOL["f32"])
        print("%s, %s: H_old moves by up to %.3g, H_new by up to %.3g (tolerance %.3g); %d of %d chains leave the sample band"
              % (cid, what, d_old.max(), d_new.max(), tol, out.sum(), out.size))
        assert max(d_old.max(), d_new.max()) > tol or out.mean() > 2 * T.MAX_OUTSIDE["f32"]


@pytest.mark.parametrize("kind", sorted(T.GRID_CASES))
def test_the_grid_stride_runs_discriminate(kind):
    """On the 17 chains compared: acceptance in [0.2, 0.9], both branches at burn + 1; the workgroup's second chain (the last one)
    does not start where its first one (chain 0) does, and the float32 oracle stays within the band on all of them."""
    case, ref = T.GRID_CASES[kind], T.grid_reference(kind)
    chains = T.grid_chains(case)
    assert chains.size == 17 and chains[-1] == case.C - 1 == T.GRID[kind] and list(chains[:8]) == list(range(8))
    q2 = _report(case.id, case, ref)
    assert 0.2 <= ref.accept.mean() <= 0.9 and (~q2).sum() >= 2 and q2.sum() >= 2
    th0 = T.inputs(case.id)[2]
    assert np.abs(th0[-1] - th0[0]).max() > 0.1 and np.abs(ref.samples[-1][-1] - ref.samples[-1][0]).max() > 0.1
    low = T.run_oracle(case, chains, dtype=np.float32)
    assert not T.outside(low.samples.astype(np.float64), ref.samples, T.KINK_TOL).any()


@pytest.mark.parametrize("kind", sorted(T.API_CASES))
def test_the_api_runs_discriminate(kind):
    case, ref = T.API_CASES[kind], T.api_reference(kind)
    q2 = _report(case.id, case, ref)
    assert 0.2 <= ref.accept.mean() <= 0.9 and (~q2).sum() >= 2 and q2.sum() >= 2
    low = T.run_oracle(case, dtype=np.float32, chain_offset=0)
    assert T.outside(low.samples.astype(np.float64), ref.samples, T.KINK_TOL).sum() <= T.KINK_MAX_CHAINS
