"""GPU: the torch-evaluated callback engine (`_GenericHMC`, hamiltorch_amd/samplers.py: torch evaluates the callable for all chains, the
kernels of csrc/hmc_pieces.hip do the rest) against oracle/hmc_oracle.py chain by chain on the same Philox streams - nothing of the
library on the reference side.  Every run is `native=False` on a closure no recogniser sees through, and hta_last_route() must name
no fused or compiled kernel.

The runs are those of tests/generic_cases.py: the (mass, burn) rows put the trajectory burn + 1 - where a rejected chain restarts from
params_init and the carried (gradient, log p) pair must be recomputed - on the capture warm-up (burn 0), inside graph replay (burn 3)
and on the first eager trajectory (burn -1).  Bounds: float64 1e-9; float32 4 x the float32 oracle's own distance from the float64
oracle, at least 2e-6 (the funnel rows 2e-4: see generic_cases.Run.bound); at most 3 % of the chains outside (a flipped accept
decision), and the acceptance rates of the others equal to the oracle's.  tests/test_generic_cases_cpu.py checks the oracle side."""
import numpy as np
import pytest
import torch

import generic_cases as G

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
GRAPHS = pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])


@pytest.fixture(scope="module")
def ht():
    import hamiltorch_amd
    assert torch.cuda.is_available()
    return hamiltorch_amd


def tt(a, dtype):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def route():
    from hamiltorch_amd import _abi
    return _abi.last_route()


def on_the_callback_route(why="native=False"):
    r = route()
    assert r.startswith("torch-evaluated callback") and why in r and "hta_" not in r, r


def closure_of(run, dtype):
    if run.split:
        return [t.closure(dtype, "cuda") for t in run.target]
    t = run.target
    return (t.logp_of if isinstance(t, G.Mixed) else t).closure(dtype, "cuda")


def sample(ht, run, dtype, fn=None, captures=True, **over):
    """sample() of a generic_cases.Run -> (rows [n, C, D], acceptance rates [C]).  captures: no capture of the run may have been
    given up (util.graph_log), or "as captured graphs" would quietly be an eager run."""
    from hamiltorch_amd import util
    del util.graph_log[:]
    fn = closure_of(run, dtype) if fn is None else fn
    if run.split:
        over.setdefault("integrator", getattr(ht.Integrator, run.split))
    out, acc = ht.sample(fn, tt(run.start(dtype), dtype), inv_mass=tt(run.inv_mass(dtype), dtype), **dict(run.kwargs(), **over))
    on_the_callback_route()
    assert len(out) == run.N - max(run.burn, -1)
    assert not (captures and util.graph_log), util.graph_log
    return torch.stack(list(out)).cpu().numpy(), acc.cpu().numpy()


def against(got, acc, ref, acc_ref, tol, what):
    """Every chain within `tol` of the reference's, at most 3 % exempt, the acceptance rates of the others equal."""
    assert got.shape == ref.shape and got.dtype == ref.dtype
    err = G.deviation(got, ref)
    bad = ~(err <= tol)
    print("%s: %d of %d chains outside %.2e; largest difference of the others %.3g; acceptance %.2f"
          % (what, bad.sum(), bad.size, tol, err[~bad].max() if (~bad).any() else np.nan, acc_ref.mean()))
    assert bad.mean() <= G.MAX_FLIPPED, "%s: %d of %d chains differ (max err %.3g, bound %.3g)" % (what, bad.sum(), bad.size, np.nanmax(err), tol)
    np.testing.assert_allclose(acc[~bad], acc_ref[~bad], atol=1e-12)
    return err


def against_oracle(got, acc, run, dtype, what=""):
    ref, info = run.oracle(dtype)
    return against(got, acc, ref, info["acc_rate"], run.bound(dtype), "%s %s %s" % (run.name, G.TAG[dtype], what))


# ---- oracle parity -------------------------------------------------------------------------------------------------------------------------
@GRAPHS
@DTYPES
@pytest.mark.parametrize("name", G.ORACLE_RUNS)
def test_sample_against_the_oracle(ht, name, dtype, graphs, monkeypatch):
    """Dense Gaussians at D = 1, 5, 11, 65, 130 and the 11-D funnel, 70 chains, 12 trajectories: as captured graphs (the first
    trajectory eager, the second the capture's warm-up, the rest replayed) and with HAMILTORCH_AMD_GRAPHS=0."""
    if not graphs:
        monkeypatch.setenv("HAMILTORCH_AMD_GRAPHS", "0")
    run = G.RUNS[name]
    got, acc = sample(ht, run, dtype)
    against_oracle(got, acc, run, dtype, "graphs" if graphs else "eager")


@DTYPES
def test_without_the_carried_pair(ht, dtype, monkeypatch):
    """HAMILTORCH_AMD_CARRY=0 evaluates (gradient, log p) at the current point afresh every trajectory; the default carries them along
    the Metropolis decisions.  At this step size the oracle rejects 30 - 70 % of the proposals, so both branches of the carry are
    used by nearly every chain.  Each against the oracle, and against each other."""
    run = G.RUNS["carry"]
    carried, acc_c = sample(ht, run, dtype)
    against_oracle(carried, acc_c, run, dtype, "carry")
    monkeypatch.setenv("HAMILTORCH_AMD_CARRY", "0")
    fresh, acc_f = sample(ht, run, dtype)
    against_oracle(fresh, acc_f, run, dtype, "no carry")
    against(fresh, acc_f, carried, acc_c, run.bound(dtype), "carry against no carry %s" % G.TAG[dtype])


@DTYPES
def test_a_run_cut_into_advance_calls(ht, dtype):
    """The engine driven as run_nuts() drives it: advance(0, 4) captures and replays, advance(4, 5) starts - eagerly - with the
    trajectory burn + 1 and captures again, advance(9, 3) is too short for a graph.  Against the uncut run and the oracle; a visible
    progress bar (verbose=True) changes nothing."""
    from hamiltorch_amd import samplers
    run = G.RUNS["chunks"]
    assert run.burn == 3 and run.N == 12
    whole, acc = sample(ht, run, dtype)
    against_oracle(whole, acc, run, dtype, "uncut")
    loud, acc_l = sample(ht, run, dtype, verbose=True)
    assert np.array_equal(loud, whole) and np.array_equal(acc_l, acc)
    eng = samplers._GenericHMC(closure_of(run, dtype))
    eng.begin(tt(run.start(dtype), dtype), run.N, run.burn, tt(run.inv_mass(dtype), dtype), run.seed, run.off)
    for n0, count in ((0, 4), (4, 5), (9, 3)):
        eng.advance(n0, count, run.L, run.eps)
    rows, rejected = eng.finish()
    cut, acc_cut = rows.cpu().numpy(), 1.0 - rejected.cpu().numpy().astype(np.float64) / run.N
    against_oracle(cut, acc_cut, run, dtype, "cut")
    against(cut, acc_cut, whole, acc, run.bound(dtype), "cut against uncut %s" % G.TAG[dtype])


# ---- the split integrators -----------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", G.SPLIT_RUNS)
def test_split_against_the_oracle(ht, name, dtype):
    """Three quadratic subsets under SPLITTING, SPLITTING_RAND (its subset order drawn on the host: never captured) and SPLITTING_KMID,
    D = 5 and 65, the three (mass, burn) rows, against O.sample_hmc(grad_fns=, logp_fns=, split_kind=)."""
    run = G.RUNS[name]
    got, acc = sample(ht, run, dtype)
    against_oracle(got, acc, run, dtype)


# ---- callables torch.func cannot batch, gradients handed in ---------------------------------------------------------------------------------
def test_the_per_chain_loop_against_the_oracle(ht):
    """A callable with a Python `if` on its argument: vmap refuses it, the engine warns and evaluates it chain by chain (9 chains,
    D = 4, float64); both sides of the branch are visited."""
    run = G.RUNS["loop"]
    with pytest.warns(UserWarning, match="not vmap-able"):
        got, acc = sample(ht, run, torch.float64, captures=False)
    against_oracle(got, acc, run, torch.float64)
    assert (got[..., 0] < 0).any() and (got[..., 0] > 0).any()


@DTYPES
def test_pass_grad_as_a_callable(ht, dtype):
    """The gradient handed in is that of ANOTHER Gaussian: the oracle integrates that gradient under the callable's log p."""
    run = G.RUNS["pass_grad_callable"]
    got, acc = sample(ht, run, dtype, pass_grad=G.PASS_GRAD_OTHER.grad_closure(dtype, "cuda"))
    against_oracle(got, acc, run, dtype)


@DTYPES
def test_pass_grad_as_a_tensor(ht, dtype):
    """A constant gradient: every kick adds the same vector (S:61-63), the energies are the callable's."""
    run = G.RUNS["pass_grad_tensor"]
    got, acc = sample(ht, run, dtype, pass_grad=tt(G.PASS_GRAD_CONST, dtype))
    against_oracle(got, acc, run, dtype)


# ---- divergence ---------------------------------------------------------------------------------------------------------------------------
@GRAPHS
def test_a_non_finite_proposal_rejects_that_chain_only(ht, graphs, monkeypatch):
    """log p is NaN outside a ball (float64).  The oracle sees non-finite proposals in most chains and finite accepted ones in every
    chain (tests/test_generic_cases_cpu.py); chain by chain the engine makes the same decisions and keeps every row finite."""
    if not graphs:
        monkeypatch.setenv("HAMILTORCH_AMD_GRAPHS", "0")
    run = G.RUNS["ball"]
    got, acc = sample(ht, run, torch.float64, captures=False)
    assert np.isfinite(got).all()
    against_oracle(got, acc, run, torch.float64)


# ---- leapfrog() ---------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("D", sorted(G.LEAPFROG))
def test_leapfrog_of_one_chain(ht, D, dtype):
    """A (D,) input keeps the torch-evaluated route: every step's (theta, p) against O.hmc_leapfrog(return_path=True) in float64 from
    the same start, D = 65 and 130 (the full-mass drift beyond D = 11), the three mass kinds.  float64: 1e-11 relative to the path's
    scale (tests/test_gpu_hmc.py); float32: 4 x the oracle's own float32 distance, at least 4 ulp of the scale."""
    dt = G.NP[dtype]
    steps, eps = G.LEAPFROG[D]
    fn = G.DenseGaussian(D).closure(dtype, "cuda")
    for mass in G.MASSES:
        th, p = G.leapfrog_start(D)
        pt, pp = ht.samplers.leapfrog(tt(th, dtype), tt(p, dtype), fn, steps=steps, step_size=eps, inv_mass=tt(G.inv_mass(mass, D, dt), dtype),
                                      sampler=ht.Sampler.HMC, integrator=ht.Integrator.EXPLICIT)
        on_the_callback_route("one chain")
        assert len(pt) == len(pp) == steps and pt[0].shape == (D,)
        wt, wp = G.leapfrog_path(D, mass, dt, np.float64)
        dist, scale = G.F32_LEAPFROG[(D, mass)]
        tol = 1e-11 * scale if dtype == torch.float64 else max(4.0 * dist, 4.0 * G.ULP32 * scale)
        err = max(np.abs(torch.stack(pt).cpu().numpy() - wt).max(), np.abs(torch.stack(pp).cpu().numpy() - wp).max())
        print("leapfrog %s D=%d %s: %.3g (bound %.3g)" % (G.TAG[dtype], D, mass, err, tol))
        assert err <= tol, (mass, err, tol)
