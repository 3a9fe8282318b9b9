"""No GPU: everything tests/test_gpu_netn_traj.py takes for granted about tests/netn_traj_cases.py, checked on the oracle alone - the
table is the one asked for, the instance every run must report follows from the launcher's rule, and every case can tell a wrong
kernel from a right one: it rejects and accepts, the Q2 reset at trajectory burn + 1 runs and is told apart from "keep current", the
float32 arithmetic does not move a chain across a ReLU kink or a Metropolis threshold, a float64 decision has room, and the diagonal
mass matters."""
import numpy as np
import pytest

import netn_traj_cases as T

RES = [T.res_case(T.NOMINAL_CUS), T.res_case(T.NOMINAL_CUS + 1)]
EDGE_CASES = {c.id: c for c in RES + [T.grid_netn_case(), T.grid_mlp3_case(2 * T.NOMINAL_CUS + 1)]}


def _report(name, case, ref):
    q2 = ref.accept[T.BURN + 1]
    print("%s: eps %g, seed %d, acceptance %.2f, %d of %d chains reject at burn + 1" % (name, case.eps, case.seed, ref.accept.mean(), (~q2).sum(), q2.size))
    return q2


def test_the_table_is_the_one_asked_for():
    """32 chains, L = 3, 7 trajectories, burn 1, chain offset 3, taus = [1 + 0.25 k], tau_out 6; the shapes, likelihoods, integrators
    and masses per id; which ids run on which route."""
    assert (T.C, T.L, T.NTRAJ, T.BURN, T.CHAIN_OFFSET, T.TAU_OUT) == (32, 3, 7, 1, 3, 6.0)
    want = {"n1": ((1, 10, 10, 1), "relu", "regression", 100, 4, "symmetric", "diag"),
            "n2": ((4, 3), "relu", "softmax", 50, 3, "rand", "none"),
            "n3": ((3, 8, 8, 8, 2), "sigmoid", "bernoulli", 35, 2, "kmid", "diag"),
            "n4": ((5, 7, 6, 3), "tanh", "softmax", 130, 1, "leapfrog", "diag"),
            "n5": ((64, 5, 1), "relu", "regression", 65, 2, "symmetric", "diag"),
            "n6": ((6, 17, 18, 1), "tanh", "regression", 24, 3, "symmetric", "diag"),
            "n7": ((2, 3, 10), "tanh", "softmax", 33, 2, "symmetric", "none"),
            "n8": ((6, 1), "relu", "bernoulli", 64, 2, "kmid", "diag"),
            "n9": ((3, 5, 2), "tanh", "regression", 300, 2, "rand", "diag"),
            "n10": ((1, 10, 10, 1), "relu", "regression", 100, 4, "symmetric", "diag"),
            "w1": ((2, 65, 3, 1), "tanh", "regression", 24, 3, "symmetric", "diag"),
            "w2": ((4, 5, 66, 1), "relu", "regression", 50, 2, "kmid", "diag"),
            "w3": ((3, 104, 4, 1), "sigmoid", "regression", 230, 1, "leapfrog", "diag"),
            "w4": ((1, 65, 2, 1), "relu", "regression", 16, 4, "rand", "none")}
    assert {k: tuple(c[1:8]) for k, c in T.CASES.items()} == want
    for c in T.CASES.values():
        assert (c.C, c.L, c.ntraj, c.tau_out) == (32, 3, 7, 6.0) and c.extra_rows == (5 if c.id == "n10" else 0)
        assert T.taus(c) == [1.0 + 0.25 * k for k in range(2 * (len(c.dims) - 1))] and (c.integ == "leapfrog") == (c.M == 1)
    assert T.CASES["n10"]._replace(id="n1", extra_rows=0) == T.CASES["n1"]
    assert T.RUNS == [("f32", "n%d" % k) for k in range(1, 10)] + [("f64", i) for i in ("n1", "n2", "n3", "n4", "n6")] \
        + [("mlp3", "w%d" % k) for k in range(1, 5)]
    assert T.WAVE_RUNS == [("w2", "n9"), ("w4", "n9"), ("w2", "n4"), ("w4", "n4")]
    assert [T.tag(*r) for r in T.WAVE_RUNS] == ["f32", "f32", "f64", "f64"]
    # the launch-edge runs
    for c in RES:
        assert tuple(c[1:8]) == ((3, 16, 16, 2), "tanh", "regression", 140, 2, "symmetric", "diag") and (c.L, c.ntraj) == (2, 4)
    assert (RES[0].C, RES[1].C) == (T.NOMINAL_CUS, T.NOMINAL_CUS + 1) and RES[0].eps == RES[1].eps and RES[0].seed == RES[1].seed
    g = T.grid_netn_case()
    assert tuple(g[1:8]) == ((1, 2, 1), "relu", "regression", 4, 2, "symmetric", "diag") and (g.L, g.ntraj, g.eps, g.C) == (2, 4, 0.2, 65537)
    assert T.n_rows(g) * g.C * T.n_params(g) == 65537 * 7 * 3
    g = T.grid_mlp3_case(2 * T.NOMINAL_CUS + 1)
    assert tuple(g[1:8]) == ((1, 65, 1, 1), "relu", "regression", 8, 2, "symmetric", "diag") and (g.L, g.ntraj, g.C) == (2, 4, 2 * T.NOMINAL_CUS + 1)


def test_the_edges_the_shapes_were_chosen_for():
    """What the table's last column says, from the shapes: sweeps of 64 PB points, remainder loops, blocks, registers."""
    pb = T.NETN_PB
    c = T.CASES["n1"]; assert pb["n1"] == 2 and c.M * c.Nb == 3 * 128 + 16 and c.Nb <= 128          # full data: sweeps, the last one ragged
    assert T.CASES["n2"].dims[-1] == 3 and len(T.CASES["n2"].dims) == 2                           # O < 4: only the remainder loop
    assert len(T.CASES["n3"].dims) == 5 and pb["n3"] == 1
    c = T.CASES["n4"]; assert pb["n4"] == 4 and c.Nb <= 256 and all(d % 4 for d in c.dims)
    c = T.CASES["n5"]; assert c.dims[0] == 64 and pb["n5"] == 2 and c.Nb == 65
    c = T.CASES["n6"]; assert T.n_params(c) == 462 and T.n_blocks(c.dims) == 40 and (40 + 15) // 16 == 3
    c = T.CASES["n7"]; assert c.dims[-1] == 10 and c.Nb < 64 and c.Nb > 32
    c = T.CASES["n8"]; assert T.n_params(c) == 7 and c.Nb == 64
    c = T.CASES["n9"]; assert pb["n9"] == 4 and 256 < c.Nb < 512 and c.dims[-1] == 2
    # mlp3 (hamiltorch_amd/csrc/mlp3_mfma.hip): eligible by a width above 64 with at most 4 inputs and 104 units; chunks of 112 points
    for cid in T.MLP3_IDS:
        c = T.CASES[cid]
        assert len(c.dims) == 4 and c.dims[-1] == 1 and c.loss == "regression" and c.dims[0] <= 4
        assert max(c.dims[1:3]) > 64 and max(c.dims[1:3]) <= 104
    assert T.CASES["w1"].Nb % 4 == 0 and T.n_params(T.CASES["w1"]) == 397 and T.CASES["w2"].Nb % 4 != 0
    c = T.CASES["w3"]; assert c.dims[1] == 104 and (c.Nb + 111) // 112 == 3 and c.Nb - 2 * 112 == 6
    c = T.CASES["w4"]; assert c.Nb < 112 and c.M == 4
    g = T.grid_mlp3_case(2 * T.NOMINAL_CUS + 1); assert g.dims[1] > 64 and T.n_params(g) == 198


def test_expected_route_is_the_launchers_rule():
    """hamiltorch_amd/csrc/netn_hmc.hip:netn_hmc restated: halve WV while Nb <= 32 WV, then PB from 4 while Nb <= 32 PB WV.  The
    residency term (every chain of the launch resident at once) decides for `res` alone: at 32 chains it never binds."""
    for route, cid in [r for r in T.RUNS if r[0] != "mlp3"] + T.WAVE_RUNS + [("f32", "n10"), ("f64", "n10")]:
        c = T.CASES[cid]
        size = 8 if T.tag(route, cid) == "f64" else 4
        wv, pb = T.WAVES[route], 4
        while wv > 1 and c.Nb <= 32 * wv:
            wv //= 2
        while pb > 1 and c.Nb <= 32 * pb * wv:
            pb //= 2
        name = "netn_hmc_kernel<%s,%d,%d>" % ("double" if size == 8 else "float", pb, wv)
        assert T.expected_route(route, cid) == name, (route, cid)
        assert T.launcher_rule(c.dims, c.Nb, c.C, T.WAVES[route], T.NOMINAL_CUS, size) == (pb, wv)      # residency does not bind
        assert T.lds_for(c.dims, pb, wv, size) <= 150 * 1024
    assert T.WAVE_PB_WV[("w2", "n9")][1] == 2 and T.WAVE_PB_WV[("w4", "n9")][1] == 4 and T.WAVE_PB_WV[("w4", "n4")][1] == 4
    g = T.grid_netn_case()
    assert T.launcher_rule(g.dims, g.Nb, g.C, 1, T.NOMINAL_CUS) == (1, 1) and T.expected_route("f32", "grid_netn") == "netn_hmc_kernel<float,1,1>"
    for cid in T.MLP3_IDS:
        assert T.expected_route("mlp3", cid) == "mlp3_mfma_kernel<%d>" % T.ACT_ID[T.CASES[cid].act]
    # res: one workgroup of <float,4,1> per CU (more than 75 KB of the CU's 150 KB), so C = CUs is resident and C = CUs + 1 is not
    d = RES[0].dims
    assert T.lds_for(d, 4, 1) == 83528 and T.lds_for(d, 4, 1) > 75 * 1024
    for cus in (T.NOMINAL_CUS, 304, 64):
        assert T.resident(d, 4, 1, cus) == cus
        assert T.launcher_rule(d, 140, cus, 1, cus) == (4, 1) and T.launcher_rule(d, 140, cus + 1, 1, cus) == (2, 1)


def test_the_unused_rows_are_behind_the_splits():
    """n10 is n1 with five rows of 1e6 appended: the same inputs otherwise, so the same oracle, and rows a kernel must never read
    as data (one of them in the full-data pass would move log p by 1e12)."""
    a, b = T.inputs("n1"), T.inputs("n10")
    assert b[0].shape[0] == a[0].shape[0] + 5 and (b[0][-5:] == 1e6).all() and (b[1][-5:] == 1e6).all()
    assert np.array_equal(b[0][:-5], a[0]) and np.array_equal(b[1][:-5], a[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert np.array_equal(T.reference("n10").samples, T.reference("n1").samples)


def test_the_inputs_are_the_ones_described():
    for cid, c in T.CASES.items():
        X, Y, th0, im = T.inputs(cid)
        n = c.M * c.Nb + c.extra_rows
        assert X.shape == (n, c.dims[0]) and X.dtype == Y.dtype == th0.dtype == np.float32 and th0.shape == (32, T.n_params(c))
        assert (im is None) == (c.mass == "none") and (im is None or (im.dtype == np.float32 and im.min() >= 0.5 and im.max() <= 1.5))
        y = Y[:c.M * c.Nb]
        if c.loss == "softmax":
            assert Y.shape == (n,) and set(np.unique(y)) == set(float(k) for k in range(c.dims[-1]))
        elif c.loss == "bernoulli":
            assert Y.shape == (n, c.dims[-1]) and set(np.unique(y)) == {0.0, 1.0}
        else:
            assert Y.shape == (n, c.dims[-1]) and np.abs(y - np.sin(X[:c.M * c.Nb].sum(1))[:, None]).max() < 0.6
        assert not any(a.flags.writeable for a in (X, Y, th0))


def _discriminates(name, case, ref, th0, f64):
    """The conditions of tests/test_mlp_traj_cases_cpu.py:test_every_case_discriminates on one oracle run."""
    q2 = _report(name, case, ref)
    assert np.isfinite(ref.samples).all() and np.isfinite(ref.h_old).all() and np.isfinite(ref.h_new[0]).all()
    assert 0.2 <= ref.accept.mean() <= 0.9
    assert (~q2).sum() >= 2 and q2.sum() >= 2
    assert np.array_equal(ref.samples[1][~q2], th0[~q2].astype(np.float64))          # the row of burn + 1 of a rejecting chain is params_init
    # "keep current" instead of the reset: the row would be the point the trajectory started from
    kept = np.abs(ref.starts[T.BURN + 1] - th0).max(axis=1)
    print("%s: %d rejecting chains started burn + 1 further than %g from params_init (smallest such distance %.3g)"
          % (name, (kept[~q2] > T.SAMPLE_TOL["f32"]).sum(), T.SAMPLE_TOL["f32"], kept[~q2][kept[~q2] > 0].min()))
    assert ((kept > T.SAMPLE_TOL["f32"]) & ~q2).sum() >= 2
    assert np.array_equal(ref.rejected, (~ref.accept).sum(0)) and ref.rejected.max() > ref.rejected.min()
    margin = T.guard_margin(ref)
    print("%s: closest decision %.3g max(1, |H|), |H| up to %.4g" % (name, margin.min(), np.abs(ref.h_old).max()))
    if f64:
        assert margin.min() >= T.GUARD


def _float32_oracle_stays(name, case, ref, chains=None):
    low = T.run_oracle(case, chains, dtype=np.float32)
    assert low.samples.dtype == np.float32
    far = T.outside(low.samples.astype(np.float64), ref.samples, T.KINK_TOL)
    print("%s: float32 oracle further than %g on %d chains (largest %.3g)" % (name, T.KINK_TOL, far.sum(), np.abs(low.samples - ref.samples).max()))
    assert far.sum() <= T.KINK_MAX_CHAINS
    return far.sum()


@pytest.mark.parametrize("cid", [c for c in T.CASES if c != "n10"])
def test_every_case_discriminates(cid):
    """The float64 oracle alone: acceptance over all chains and trajectories in [0.2, 0.9]; at trajectory burn + 1 at least 2 chains
    reject (their row is params_init again) and at least 2 accept; at least 2 of the rejecting ones had moved by more than the sample
    band before (or their reset could not be told from keeping the current point); the float32-state oracle is further than 5e-4
    from the float64 one on at most 1 of the 32 chains; on a float64 route no decision lies within GUARD max(1, |H|) of its
    threshold."""
    case, ref = T.CASES[cid], T.reference(cid)
    assert ref.samples.shape == (T.n_rows(case), case.C, T.n_params(case))
    _discriminates(cid, case, ref, T.inputs(cid)[2], cid in T.F64_IDS)
    _float32_oracle_stays(cid, case, ref)


@pytest.mark.parametrize("cid", [c for c in T.CASES if T.CASES[c].mass == "diag" and c != "n10"] + sorted(k for k, c in EDGE_CASES.items()))
def test_the_diagonal_mass_matters(cid):
    """The oracle run again without the diagonal mass (what a kernel computes that ignores inv_mass and mass_factor): an energy of
    trajectory 0 leaves the float32 tolerance (the GPU test exempts no chain there) or more than twice the 7 % of the chains the
    sample band exempts leave it."""
    case = T.ALL_CASES[cid]
    chains = T.grid_chains(case) if cid in EDGE_CASES else None
    ref = T.grid_reference(cid) if cid in EDGE_CASES else T.reference(cid)
    bare = T.run_oracle(case, chains, mass=None)
    tol = T.ENERGY_TOL["f32"] * max(1.0, np.abs(ref.h_old[0]).max(), np.abs(ref.h_new[0]).max())
    d_old, d_new = np.abs(bare.h_old[0] - ref.h_old[0]), np.abs(bare.h_new[0] - ref.h_new[0])
    out = T.outside(bare.samples, ref.samples, T.SAMPLE_TOL["f32"])
    print("%s without its mass: H_old moves by up to %.3g, H_new by up to %.3g (tolerance %.3g); %d of %d chains leave the sample band"
          % (cid, d_old.max(), d_new.max(), tol, out.sum(), out.size))
    assert max(d_old.max(), d_new.max()) > tol and out.mean() > 2 * T.MAX_OUTSIDE["f32"]


@pytest.mark.parametrize("cid", sorted(EDGE_CASES))
def test_the_launch_edge_runs_discriminate(cid):
    """On the 17 chains compared (the first 8 and the last 9): the same conditions; the float32 oracle stays within the band on all
    but at most one; in a grid-stride run the workgroup's second chain (the last one) does not start where its first (chain 0) does."""
    case, ref = EDGE_CASES[cid], T.grid_reference(cid)
    chains = T.grid_chains(case)
    assert chains.size == 17 and chains[-1] == case.C - 1 and list(chains[:8]) == list(range(8)) and len(set(chains)) == 17
    th0 = T.inputs(cid)[2]
    _discriminates(cid, case, ref, th0[chains], False)
    assert np.abs(th0[-1] - th0[0]).max() > 0.1 and np.abs(ref.samples[-1][-1] - ref.samples[-1][0]).max() > 0.1
    _float32_oracle_stays(cid, case, ref, chains)
    assert T.max_outside("f32", 17) == 1 and T.max_outside("f32", 32) == 2 and T.max_outside("f64", 32) == 0
