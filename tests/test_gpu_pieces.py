"""GPU: the state kernels of the torch-evaluated callback route (csrc/hmc_pieces.hip) one by one through hamiltorch_amd/_abi.py against
plain numpy in float64 - O.kinetic / O.hmc_hamiltonian, one explicit kick/drift step, O.philox_normals with an explicit factor,
O.mh_accept with the update rule of O.sample_chain_driver - on the cases of tests/generic_cases.py: every lane-group size of the
energy and select kernels (D = 1 .. 257), batches whose last block is partly idle (C = 1, 37, 70), the three mass kinds and a
NON-symmetric dense matrix for the drift, and one case beyond every grid-stride limit of the launch code.

Bounds (generic_cases.py): float64 1e-12 relative to the case's scale; float32 4 x the distance of the same numpy formula in float32
from its float64 value, at least 4 ulp of the scale - measured on the CPU (tests/test_generic_cases_cpu.py), never on the GPU.  The
Metropolis select copies state, it does no arithmetic on it: decisions, states, rows, counts and accept bytes are compared exactly."""
import numpy as np
import pytest
import torch

import generic_cases as G
import hmc_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
DS = pytest.mark.parametrize("D", G.PIECE_D)


@pytest.fixture(scope="module")
def abi():
    from hamiltorch_amd import _abi
    assert torch.cuda.is_available()
    _abi.load()
    return _abi


def tt(a, dtype=None):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def bound(dtype, name, mass, D, C, scale):
    return G.F64_PIECE * max(1.0, scale) if dtype == torch.float64 else G.f32_bound(name, mass, D, C)


def worst(got, ref):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape
    return float(np.abs(got.astype(np.float64) - ref).max())


def masses_at(D, extra=()):
    return [m for m in G.MASSES + tuple(extra) if D <= G.FULL_MAX_D or m in ("none", "diag")]


# ---- hta_hamiltonian ---------------------------------------------------------------------------------------------------------------------
@DTYPES
@DS
def test_hamiltonian(abi, dtype, D):
    """H = -log p + p^T M^-1 p / 2 against O.hmc_hamiltonian (O.kinetic with log p = None) in float64: G = 1 .. 64 lanes per chain, a lane
    that loops 3 and 5 times with a ragged last pass (D = 130, 257), the full-mass branch up to D = 130."""
    dt = G.NP[dtype]
    for mass in masses_at(D):
        im = G.inv_mass(mass, D, dt)
        for C in G.PIECE_C:
            x = G.piece_inputs(D, C, dt)
            x64 = {k: v.astype(np.float64) for k, v in x.items()}
            im64 = None if im is None else im.astype(np.float64)
            want, _ = O.hmc_hamiltonian(x64["theta"], x64["p"], lambda th: x64["logp"], im64)
            kin = O.kinetic(x64["p"], im64)
            tol = bound(dtype, "hamiltonian", mass, D, C, np.abs(want).max())
            for logp, ref in ((tt(x["logp"]), want), (None, kin)):
                H = torch.full((C,), float("nan"), dtype=dtype, device="cuda")
                abi.hamiltonian(tt(x["p"]), logp, G.KIND[mass], tt(im), H)
                err = worst(H, ref)
                print("hamiltonian %s D=%d C=%d %s logp=%s: %.3g (bound %.3g)" % (G.TAG[dtype], D, C, mass, logp is not None, err, tol))
                assert err <= tol, (mass, C, err, tol)


# ---- hta_kick_drift ----------------------------------------------------------------------------------------------------------------------
def kick_drift_forms(abi, dtype, D, C, mass):
    """The three call forms of the engine and a negative kick, each against one explicit numpy step in float64."""
    dt = G.NP[dtype]
    im = G.inv_mass(mass, D, dt)
    x = G.piece_inputs(D, C, dt)
    for kick, drift, with_grad in ((G.KICK, G.DRIFT, True), (G.KICK, 0.0, True), (0.0, G.DRIFT, False), (-G.KICK, 0.0, True)):
        th, p = tt(x["theta"]), tt(x["p"])
        abi.kick_drift(th, p, tt(x["grad"]) if with_grad else None, kick, drift, G.KIND[mass], tt(im))
        wt, wp = G.ref_kick_drift(x, im, kick, drift, with_grad, np.float64)
        scale = max(np.abs(wt).max(), np.abs(wp).max())
        tol = bound(dtype, "kick_drift", mass, D, C, scale)
        err = max(worst(th, wt), worst(p, wp))
        print("kick_drift %s D=%d C=%d %s kick=%g drift=%g: %.3g (bound %.3g)" % (G.TAG[dtype], D, C, mass, kick, drift, err, tol))
        assert err <= tol, (mass, C, kick, drift, err, tol)
        if drift == 0.0:
            assert torch.equal(th, tt(x["theta"])), "a kick without a drift changed theta"
        if not with_grad:
            assert torch.equal(p, tt(x["p"])), "a drift without a kick changed p"


@DTYPES
@DS
def test_kick_drift(abi, dtype, D):
    """none, diag, full and the NON-symmetric dense matrix (M^-1 p = p @ inv_mass.T, the oracle's _apply_inv_mass: with the two
    indices of inv_mass swapped the drift is another vector)."""
    for mass in masses_at(D, ("nonsym",)):
        for C in G.PIECE_C:
            kick_drift_forms(abi, dtype, D, C, mass)


# ---- hta_momentum_resample ---------------------------------------------------------------------------------------------------------------
def resample_case(abi, dtype, mass, D, C):
    dt = G.NP[dtype]
    mf = G.factor(mass, D, dt)
    z = O.philox_normals(G.RS_SEED, G.RS_OFF + np.arange(C), G.RS_DRAW, D, dtype=np.float64)
    mf64 = None if mf is None else mf.astype(np.float64)
    want = z if mf is None else (mf64 * z if mf.ndim == 1 else z @ mf64.T)
    p = torch.full((C, D), float("nan"), dtype=dtype, device="cuda")
    abi.momentum_resample(p, G.KIND[mass], tt(mf), G.RS_SEED, G.RS_OFF, G.RS_DRAW)
    tol = bound(dtype, "resample", mass, D, C, np.abs(want).max())
    err = worst(p, want)
    print("resample %s D=%d C=%d %s: %.3g (bound %.3g)" % (G.TAG[dtype], D, C, mass, err, tol))
    assert err <= tol, (mass, D, C, err, tol)
    return p


@DTYPES
@pytest.mark.parametrize("D", G.RESAMPLE_D)
def test_momentum_resample_with_an_explicit_factor(abi, dtype, D):
    """p = factor . z against O.philox_normals and the factor applied in numpy: a diagonal factor that is not 1, a lower-triangular
    one at D = 65, 129, 257 (blocks of 64, 128, 256 threads, the last partly idle).  The device-counter form draws the same bits."""
    for mass in G.MASSES:
        for C in G.PIECE_C:
            p = resample_case(abi, dtype, mass, D, C)
        q = torch.empty_like(p)
        abi.momentum_resample_at(q, G.KIND[mass], tt(G.factor(mass, D, G.NP[dtype])), G.RS_SEED, G.RS_OFF,
                                 torch.tensor([G.RS_DRAW], dtype=torch.int32, device="cuda"))
        assert torch.equal(p, q)


# ---- hta_mh_select / hta_mh_select_at ----------------------------------------------------------------------------------------------------
def select_case(abi, dtype, D, C, n, with_row, with_acc, with_lp):
    dt = G.NP[dtype]
    burn = G.MH_BURN
    rng = np.random.default_rng(40 + D)
    cur, prop, init = (rng.standard_normal((70, D))[:C].astype(dt) for _ in range(3))
    Ho, Hn, lp, klass = G.mh_inputs(C, dt)
    u = G.mh_uniform(n, C, dt)
    rej0 = np.arange(C, dtype=np.int32)
    acc, new, row, rej = G.mh_expected(cur, prop, init, Ho, Hn, lp if with_lp else None, n, burn, u, rej0)
    # at most one random-class chain may lie in the guard band; the CPU tests show that none does, so none is left out here
    assert (G.mh_margin(Ho, Hn, u)[klass == "x"] >= G.MH_GUARD).all()
    S = 4
    want_samples = np.full((S, C, D), G.MH_SENTINEL, dt)
    if with_row and row is not None:
        want_samples[n - burn] = row
    out = []
    for at in (False, True):
        c, samples = tt(cur), torch.full((S, C, D), G.MH_SENTINEL, dtype=dtype, device="cuda")
        r, a = tt(rej0), (torch.full((C,), 9, dtype=torch.uint8, device="cuda") if with_acc else None)
        args = (tt(Ho), tt(Hn), tt(lp) if with_lp else None)
        if at:
            abi.mh_select_at(c, tt(prop), tt(init), *args, samples if with_row else None, r, a,
                             torch.tensor([n], dtype=torch.int32, device="cuda"), burn, G.MH_SEED, G.MH_OFF)
        else:
            # n <= burn: the engine passes no row; a row passed all the same must stay untouched
            abi.mh_select(c, tt(prop), tt(init), *args, samples[max(n - burn, 0)] if with_row else None, r, a, n, burn, G.MH_SEED, G.MH_OFF)
        got = (c.cpu().numpy(), samples.cpu().numpy(), r.cpu().numpy(), None if a is None else a.cpu().numpy())
        what = "%s D=%d C=%d n=%d row=%s acc=%s lp=%s at=%s" % (G.TAG[dtype], D, C, n, with_row, with_acc, with_lp, at)
        if with_acc:
            assert np.array_equal(got[3], acc.astype(np.uint8)), ("decisions", what, np.flatnonzero(got[3] != acc))
        assert np.array_equal(got[2], rej.astype(np.int32)), ("reject counts", what)
        assert np.array_equal(got[0], new), ("current state", what)
        assert np.array_equal(got[1], want_samples), ("sample rows", what)
        out.append(got)
    for g0, g1 in zip(*out):                                   # the device-counter form, bit for bit
        assert g0 is None or np.array_equal(g0, g1)
    return acc, klass


@DTYPES
@DS
def test_mh_select(abi, dtype, D):
    """cur, prop and init distinct, reject counts starting at arange(C), rows pre-filled with a sentinel, n = burn - 1 .. burn + 2
    (a reject at burn + 1 restarts from init: SURVEY Q2), with every output and without the optional ones, the five classes of chains
    of generic_cases.mh_inputs (C = 70 holds all of them; C = 1 is a sure accept); both entry points."""
    for C in G.PIECE_C:
        for n in G.MH_N:
            acc, klass = select_case(abi, dtype, D, C, n, True, True, True)
            if C == 70:
                assert acc[klass == "a"].all() and not acc[klass == "r"].any() and not acc[klass == "n"].any()
                assert 0 < acc[klass == "x"].sum() < (klass == "x").sum()
    for n in G.MH_N:
        select_case(abi, dtype, D, 70, n, False, False, False)
        select_case(abi, dtype, D, 37, n, True, False, False)
        select_case(abi, dtype, D, 37, n, False, True, True)


# ---- beyond the grid-stride limits (float32) -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", G.MASSES)
def test_kick_drift_beyond_one_grid(abi, mass):
    """C D = 539 700 elements on 2048 blocks of 256 threads: kick_drift_kernel and drift_full_kernel stride; every element compared."""
    C, D = G.STRIDE_KICK
    assert C * D > 2048 * 256
    kick_drift_forms(abi, torch.float32, D, C, mass)


@pytest.mark.parametrize("mass", ["none", "diag"])
def test_momentum_resample_beyond_one_grid(abi, mass):
    C, D = G.STRIDE_RESAMPLE
    assert C * ((D + 3) // 4) > 2048 * 256
    resample_case(abi, torch.float32, mass, D, C)


def test_full_mass_resample_beyond_4096_chains(abi):
    C, D = G.STRIDE_RESAMPLE_FULL
    assert C > 4096
    resample_case(abi, torch.float32, "full", D, C)


@DTYPES
def test_run_begin_beyond_one_grid(abi, dtype):
    """cur <- init, row 0 <- init, reject counts <- 0 on more words than 4096 blocks of 256 threads hold; nothing beyond row 0."""
    C, D = G.STRIDE_RESAMPLE
    assert C * D > 4096 * 256
    init = torch.tensor(G.piece_inputs(D, C, G.NP[dtype])["theta"], device="cuda")
    cur = torch.full_like(init, G.MH_SENTINEL)
    samples = torch.full((2, C, D), G.MH_SENTINEL, dtype=dtype, device="cuda")
    rej = torch.arange(1, C + 1, dtype=torch.int32, device="cuda")
    abi.run_begin(init, cur, samples[0], rej)
    assert torch.equal(cur, init) and torch.equal(samples[0], init) and int(rej.abs().max()) == 0
    assert bool((samples[1] == G.MH_SENTINEL).all())
    rej.fill_(7)
    abi.run_begin(init, cur, None, None)
    assert torch.equal(cur, init) and bool((rej == 7).all())
