"""GPU: tuning key "quad_prop" (csrc/hmc_gauss_quad_dev.hpp: quad_body PROP, the ..._prop_kernel twins; csrc/quad_prop.hpp) - every
launch form of the quad route applies a trajectory's L leapfrog steps as one precomputed linear map.  The map is the steps' own
arithmetic run in float64 and rounded once, so against the step-by-step instances ("quad_prop" = 0) the results are the same to
rounding, not bit for bit.

(1) "quad_prop" 1 against 0, chain by chain: rows and the final state inside row_band (tests/gauss_traj_cases.py: 2e-4 max(1, |want|)),
    equal reject counts.  A chain whose Metropolis decision sits on its threshold may flip under ANY change of rounding and then
    differs everywhere behind the flip; the float64 oracle says which chains can: a chain is CLEAR when its guard_margin
    (|min(0, dH) - log u| / max(1, |H|)) is above the band at every trajectory.  No clear chain may differ, and of all chains of a
    parametrised case at most 1 %.
(2) "quad_prop" = 1 against oracle/hmc_oracle.py:sample_hmc (float64, the same Philox draws) at the bands of tests/test_gpu_hmc.py:
    rows within 2e-4, reject counts equal, on all but 1 % of the chains - again none of them a clear chain.
    Shapes of (1) and (2): D = 1 .. 4; C = 5, 15, 16, 17, 65 and 8, 24, 40 (the dispatcher takes the one-launch route only for
    C % 8 == 0: 8, 16, 24, 40 reach the default 512-thread twin with its four chains per block, the others the two-launch twin);
    L = 1, 7, 25, 100; burn = -1, 0, 2, N - 1; N = 1, 3, 4, 5, 36, 37, 68: every group shape of quad_local_groups (singles, the lead
    group of 4, full passes of 32, groups of 4 behind them, the Q2 single at the front, behind the lead group and nowhere).  One oracle
    run per (D, L, burn) on 65 chains and 68 trajectories serves every shape: chains are independent, a shorter run is a prefix, and a
    run that is all burn-in walks the states of the burn = -1 run (its only Q2 reset, at trajectory 0, resets to the start itself).
    Plus C = 1024, N = 40.
(3) A diverging step size: every proposal is rejected - rows, final state and reject counts torch.equal to that outcome.
(4) "quad_prop_chains" 4 / 8 / 16 and "quad_prop_sweep" 0 / 1 / 2 move records between blocks and lanes, not bits: torch.equal.
(5) Form against form at "quad_prop" = 0, so that the step-by-step partners keep their GPU coverage: one small shape per key,
    torch.equal - quad_fused, quad_rows, quad_local, quad_wide, quad_lead, each 0 against 1."""
import functools

import numpy as np
import pytest
import torch

import hmc_oracle as O

pytestmark = pytest.mark.gpu

SEED, EPS = 13, 0.3
CHAINS = [5, 15, 16, 17, 65, 8, 24, 40]
LS = [1, 7, 25, 100]
N_TRAJ = [1, 3, 4, 5, 36, 37, 68]
CMAX, NMAX = 65, 68


def burns_of(N):
    """burn = -1, 0, 2 and N - 1, as far as burn < N"""
    return sorted({b for b in (-1, 0, 2, N - 1) if b <= N - 1})


def dev():
    return torch.device("cuda:0")


def rand_spd(D, seed, lo=0.5, hi=2.0):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    P = (Q * np.linspace(lo, hi, D)) @ Q.T
    return 0.5 * (P + P.T)


@functools.lru_cache(maxsize=None)
def model(D, C=CMAX):
    """(P, mu, th0[C, D]) in float32, read-only; the first chains of a larger C are those of a smaller one."""
    P = rand_spd(D, 8 + D).astype(np.float32)
    P = 0.5 * (P + P.T)
    mu = np.linspace(-0.5, 0.5, D).astype(np.float32)
    th0 = (mu + 0.5 * O.philox_normals(SEED, np.arange(C), 0, D, O.PURPOSE_INIT, dtype=np.float64)).astype(np.float32)
    for a in (P, mu, th0):
        a.setflags(write=False)
    return P, mu, th0


@functools.lru_cache(maxsize=None)
def oracle(D, L, burn, C=CMAX, N=NMAX, eps=EPS):
    """(rows[N - burn, C, D], accept[N, C], margin[N, C]) of the float64 oracle; computed once, shared, read-only."""
    P, mu, th0 = model(D, C)
    tg = O.GaussianTarget(mu.astype(np.float64), P.astype(np.float64), 0.0)
    ids = np.arange(C)
    ret, info = O.sample_hmc(tg, th0.astype(np.float64), N, L, np.float64(np.float32(eps)), burn, None, O.PhiloxDraws(SEED, ids, np.float64))
    ho, hn, acc = np.stack(info["h_old"]), np.stack(info["h_new"]), np.stack(info["accept"])
    log_u = np.stack([np.log(O.PhiloxDraws(SEED, ids, np.float64).mh_uniform(k).astype(np.float64)) for k in range(N)])
    margin = np.abs(np.minimum(0.0, ho - hn) - log_u) / np.maximum(1.0, np.maximum(np.abs(ho), np.abs(hn)))
    out = (np.stack(ret), acc, margin)
    for a in out:
        a.setflags(write=False)
    return out


def expected(D, L, burn, C, N, Cmax=CMAX, Nmax=NMAX):
    """(rows[N - burn, C, D], cur[C, D], rejected[C], margin[C]) of a run of N trajectories on the first C chains, from the shared runs."""
    if burn == N - 1:                               # all burn-in: the states of the burn = -1 run, no stored row but the start
        rows, acc, margin = oracle(D, L, -1, Cmax, Nmax)
        return rows[:1, :C], rows[N, :C], (~acc[:N, :C]).sum(0), margin[:N, :C].min(0)
    rows, acc, margin = oracle(D, L, burn, Cmax, Nmax)
    r = rows[:N - max(burn, -1), :C]
    return r, r[-1], (~acc[:N, :C]).sum(0), margin[:N, :C].min(0)


def run(D, C, N, L, burn, keys, eps=EPS, Cmodel=CMAX, prepared=True):
    """(rows[N - burn, C, D] with row 0 = the start, cur, rejected) in numpy, through the C ABI under `keys`; the route is asserted."""
    from hamiltorch_amd import _abi
    _abi.reset_tuning()
    for k, v in keys.items():
        _abi.set_tuning(k, v)
    P, mu, th0 = model(D, Cmodel)
    th0 = torch.tensor(th0[:C], device=dev())
    Pd, mud = torch.tensor(P, device=dev()), torch.tensor(mu, device=dev())
    ws = torch.zeros(_abi.gaussian_workspace_bytes(C, D, N, 4), dtype=torch.uint8, device=dev())
    if prepared:
        _abi.hmc_gaussian_prepare(th0, Pd, 0, None, C, D, N, ws)
    samples = torch.zeros(N - max(burn, -1), C, D, device=dev())
    samples[0] = th0
    rej = torch.zeros(C, dtype=torch.int32, device=dev())
    cur = th0.clone()
    _abi.hmc_gaussian_sample(cur, th0, Pd, mud, 0.0, 0, None, None, L, eps, N, 0, burn, SEED, 0, samples, rej, workspace=ws)
    one_launch = prepared and C % 8 == 0 and N >= 8 and keys.get("quad_fused", 1)
    want = "hmc_gauss_quad_fused_kernel<%d" % D if one_launch else "hmc_gauss_quad_kernel<%d" % D
    assert _abi.last_route().startswith(want), (C, N, _abi.last_route())
    torch.cuda.synchronize()
    if one_launch:
        word = _abi.hmc_gaussian_status_word(ws, C, D, N, 4)
        assert word is not None and int(word) == 0
    _abi.hmc_gaussian_forget(ws)
    return samples.cpu().numpy(), cur.cpu().numpy(), rej.cpu().numpy().astype(np.int64)


@pytest.fixture(autouse=True)
def _restore_keys():
    from hamiltorch_amd import _abi
    try:
        yield
    finally:
        _abi.reset_tuning()


def test_the_keys_exist_and_reset_to_their_defaults():
    from hamiltorch_amd import _abi
    _abi.reset_tuning()
    assert _abi.get_tuning("quad_prop") == 1
    dflt = {k: _abi.get_tuning(k) for k in ("quad_prop", "quad_prop_chains", "quad_prop_sweep")}
    for k in dflt:
        _abi.set_tuning(k, dflt[k] + 1)
    _abi.reset_tuning()
    assert {k: _abi.get_tuning(k) for k in dflt} == dflt


def _differs(a, b, band):
    """chain by chain: rows or final state further apart than `band`, or another reject count"""
    with np.errstate(invalid="ignore"):
        return ~((np.abs(a[0] - b[0]).max(axis=(0, 2)) <= band) & (np.abs(a[1] - b[1]).max(axis=1) <= band) & (a[2] == b[2]))


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_propagated_against_stepwise_and_against_the_oracle(D, L):
    n_chains = n_flip = n_off = n_clear = 0
    worst_pair = worst_oracle = 0.0
    for N in N_TRAJ:
        for burn in burns_of(N):
            for C in CHAINS:
                rows, cur, rej, margin = expected(D, L, burn, C, N)
                prop = run(D, C, N, L, burn, dict(quad_prop=1))
                step = run(D, C, N, L, burn, dict(quad_prop=0))
                assert np.isfinite(prop[0]).all() and np.isfinite(prop[1]).all()
                band = 2e-4 * max(1.0, float(np.abs(step[0]).max()))
                clear = margin > band
                flip = _differs(prop, step, band)
                off = _differs(prop, (rows, cur, rej), 2e-4)
                what = "D=%d L=%d N=%d burn=%d C=%d" % (D, L, N, burn, C)
                assert not (flip & clear).any(), "%s: a clear chain differs between quad_prop 1 and 0" % what
                assert not (off & clear).any(), "%s: a clear chain differs from the oracle" % what
                ok = ~flip
                if ok.any():
                    worst_pair = max(worst_pair, float(np.abs(prop[0] - step[0])[:, ok].max()))
                if (~off).any():
                    worst_oracle = max(worst_oracle, float(np.abs(prop[0] - rows)[:, ~off].max()))
                n_chains += C; n_flip += int(flip.sum()); n_off += int(off.sum()); n_clear += int(clear.sum())
    print("D=%d L=%d: %d chains (%d clear), %d differ between quad_prop 1 and 0, %d from the oracle; largest row difference of the others "
          "%.3g (pair), %.3g (oracle)" % (D, L, n_chains, n_clear, n_flip, n_off, worst_pair, worst_oracle))
    assert n_flip <= 0.01 * n_chains and n_off <= 0.01 * n_chains
    assert 2 * n_clear >= n_chains          # (the classification must not excuse most of what is compared)


def test_propagated_against_the_oracle_at_1024_chains():
    D, L, C, N = 3, 25, 1024, 40
    for burn in (-1, 2):
        rows, cur, rej, margin = expected(D, L, burn, C, N, C, N)
        prop = run(D, C, N, L, burn, dict(quad_prop=1), Cmodel=C)
        step = run(D, C, N, L, burn, dict(quad_prop=0), Cmodel=C)
        band = 2e-4 * max(1.0, float(np.abs(step[0]).max()))
        clear = margin > band
        flip, off = _differs(prop, step, band), _differs(prop, (rows, cur, rej), 2e-4)
        print("burn=%d: %d of %d chains clear, %d differ between quad_prop 1 and 0, %d from the oracle" % (burn, clear.sum(), C, flip.sum(), off.sum()))
        assert not (flip & clear).any() and not (off & clear).any()
        assert flip.mean() <= 0.01 and off.mean() <= 0.01


@pytest.mark.parametrize("C", [16, 17])
@pytest.mark.parametrize("L", [7, 100])
def test_a_diverging_step_size_rejects_everything(C, L):
    """eps sqrt(lam) > 2 on every coordinate (lam >= 0.5, eps = 3): the map's coefficients grow with L until they overflow to infinity;
    either way the energy difference is -inf or NaN, which rejects.  The outcome is exact: every row the start, every count N."""
    D, N = 3, 36
    for burn in (-1, 2):
        for prop in (1, 0):
            rows, cur, rej = run(D, C, N, L, burn, dict(quad_prop=prop), eps=3.0)
            th0 = model(D)[2][:C]
            assert np.array_equal(rows, np.broadcast_to(th0, rows.shape)), (prop, burn)
            assert np.array_equal(cur, th0) and np.array_equal(rej, np.full(C, N)), (prop, burn)


@pytest.mark.parametrize("D", [1, 2, 3])
def test_chains_per_block_and_sweeps_change_no_byte(D):
    for C in (8, 16, 24, 40):
        for N, burn in ((68, 2), (37, -1), (9, 3)):
            base = run(D, C, N, 25, burn, dict(quad_prop=1))
            for keys in (dict(quad_prop_chains=4), dict(quad_prop_chains=8), dict(quad_prop_chains=16), dict(quad_prop_chains=16, quad_prop_sweep=1),
                         dict(quad_prop_chains=16, quad_prop_sweep=2), dict(quad_prop_chains=4, quad_prop_sweep=1), dict(quad_prop_chains=8, quad_prop_sweep=2)):
                got = run(D, C, N, 25, burn, dict(quad_prop=1, **keys))
                for x, y in zip(base, got):
                    assert np.array_equal(x, y), (D, C, N, burn, keys)


@pytest.mark.parametrize("key", ["quad_fused", "quad_rows", "quad_local", "quad_wide", "quad_lead"])
def test_stepwise_forms_stay_bit_identical_to_one_another(key):
    """"quad_prop" = 0: the form with `key` = 1 against `key` = 0, everything else at its default."""
    D, C, N, L, burn = 3, 24, 41, 25, 3
    on = run(D, C, N, L, burn, {"quad_prop": 0, key: 1})
    off = run(D, C, N, L, burn, {"quad_prop": 0, key: 0})
    for x, y in zip(on, off):
        assert np.array_equal(x, y), key
    assert np.isfinite(on[0]).all()
