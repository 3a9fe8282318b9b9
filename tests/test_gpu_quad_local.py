"""GPU: tuning key "quad_local" - the fused quad launch whose draw records are made by producer waves of the consumer's own block and
handed over through LDS (csrc/hmc_gauss_quad_dev.hpp: hmc_gauss_quad_local_kernel) against the launch whose records come from producer
blocks through memory ("quad_local" = 0), both with row waves ("quad_rows" = 1).  A producer lane runs the cross-block producer's
arithmetic (quad_make_record) and the groups of trajectories do not change any of it, so samples, reject counts and the final state
are equal BIT FOR BIT (torch.equal) - over every compiled instance, partial waves and blocks, every shape of the group sequence,
launches chunked over `traj_offset` and chains sharded over `chain_offset`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ht():
    import hamiltorch_amd
    assert torch.cuda.is_available()
    return hamiltorch_amd


def dev():
    return torch.device("cuda:0")


def rand_spd(D, seed, lo=0.5, hi=2.0):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    P = (Q * np.linspace(lo, hi, D)) @ Q.T
    return 0.5 * (P + P.T)


def _target(ht, P, mu):
    return ht.GaussianTarget(torch.tensor(mu, dtype=torch.float32, device=dev()), precision=torch.tensor(P, dtype=torch.float32, device=dev()),
                             normalized=False)


def _run(t, th0, N, L, burn, local, eps=0.3, seed=13, chunks=None, off=0):
    """(samples, reject counts, final state) of N trajectories through the C ABI on a prepared workspace, `chunks`: the trajectories
    per launch (one launch of N when absent)"""
    from hamiltorch_amd import _abi
    C, D = th0.shape
    chunks = chunks or [N]
    assert sum(chunks) == N
    _abi.set_tuning("quad_rows", 1)
    _abi.set_tuning("quad_local", local)
    ws = torch.zeros(_abi.gaussian_workspace_bytes(C, D, max(chunks), 4), dtype=torch.uint8, device=dev())
    _abi.hmc_gaussian_prepare(th0, t.precision, 0, None, C, D, max(chunks), ws)
    nrow = N - max(burn, 0) + 1
    samples = torch.zeros(nrow, C, D, device=dev())
    rej = torch.zeros(C, dtype=torch.int32, device=dev())
    cur = th0.clone()
    start = 0
    for n in chunks:
        _abi.hmc_gaussian_sample(cur, th0, t.precision, t.mean, t.log_norm, 0, None, None, L, eps, n, start, burn, seed, off, samples, rej,
                                 workspace=ws)
        assert _abi.last_route().startswith("hmc_gauss_quad_fused_kernel<%d" % D), _abi.last_route()
        start += n
    torch.cuda.synchronize()
    word = _abi.hmc_gaussian_status_word(ws, C, D, max(chunks), 4)
    assert word is not None and int(word) == 0
    _abi.hmc_gaussian_forget(ws)
    return samples.cpu(), rej.cpu(), cur.cpu()


def _assert_same(a, b, what):
    for x, y, name in zip(a, b, ("samples", "reject counts", "final state")):
        assert torch.equal(x, y), "%s: %s differ" % (what, name)
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[2]).all()


def _model(ht, D, C, L):
    rng = np.random.default_rng(100 * D + L)
    mu = rng.normal(size=D)
    t = _target(ht, rand_spd(D, 8 + D), mu)
    th0 = torch.tensor(mu + rng.normal(size=(C, D)), dtype=torch.float32, device=dev())
    return t, th0


@pytest.fixture(autouse=True)
def _restore_keys():
    from hamiltorch_amd import _abi
    try:
        yield
    finally:
        _abi.reset_tuning()


# every compiled instance (L = 25, 10, 5) and the any-L one (7) at D = 1 ... 3; 16 chains are exactly one integrating wave, 24 a partial
# one (its block integrates the last chain again and stores nothing for the lanes past C), 32 two blocks, 1040 past the 1024 the
# cross-block launch scales its producers by.  (D <= 3: 4-float records, the fused launch wants C % 8 == 0.)
@pytest.mark.parametrize("C", [16, 24, 32, 1040])
@pytest.mark.parametrize("L", [25, 10, 5, 7])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_local_records_are_bit_identical_over_instances_and_chain_counts(ht, D, L, C):
    t, th0 = _model(ht, D, C, L)
    N, burn = 45, 3
    _assert_same(_run(t, th0, N, L, burn, 1), _run(t, th0, N, L, burn, 0), "D=%d L=%d C=%d" % (D, L, C))


# the group sequence at L = 25 (lead group of 4, passes of 32, tail passes of 4, single ones): 8 = the route's minimum (4 + 4),
# 37 = 4 + 32 + 1, 71 = 4 + 32 + 32 + 3 x 1; burn = 5: the burn-in phase is 4 + 1 + 1 and the Q2 trajectory opens the stored phase as
# a group of its own; burn = -1 and 0: no burn-in phase / its single trajectory in front of the Q2 one
@pytest.mark.parametrize("N,burn", [(8, -1), (37, -1), (71, -1), (71, 5), (37, 0), (8, 5), (40, 39)])
def test_local_group_sequences(ht, N, burn):
    t, th0 = _model(ht, 3, 48, 25)
    _assert_same(_run(t, th0, N, 25, burn, 1), _run(t, th0, N, 25, burn, 0), "N=%d burn=%d" % (N, burn))


@pytest.mark.parametrize("L,chunks", [(25, [41, 41]), (10, [23, 23, 23]), (25, [8, 8, 8, 8, 8])])
def test_local_launches_chunked_over_traj_offset(ht, L, chunks):
    """Launches over `traj_offset`: each launch starts its own group sequence and the records do not notice - bit for bit the
    cross-block launch's chunked run.  Against ONE launch the chunked run agrees to rounding only, on either launch: on the
    eigenbasis route the state crosses a launch boundary as q = mu + Q y (tests/test_gpu_hmc.py::test_chunked_launches_equal_single_launch,
    whose band this takes: 2e-5, at most 2 % of the chains on a decision that rounding moved).
    (Equal chunks: a prepared workspace serves launches of the trajectory count it was prepared for.)"""
    t, th0 = _model(ht, 3, 40, L)
    N = sum(chunks)
    for burn in (-1, 12):
        chunked = _run(t, th0, N, L, burn, 1, chunks=chunks)
        _assert_same(chunked, _run(t, th0, N, L, burn, 0, chunks=chunks), "chunked, burn=%d" % burn)
        one = _run(t, th0, N, L, burn, 1)
        err = (chunked[0] - one[0]).abs().amax(dim=(0, 2))
        print("chunked against one launch, burn=%d: largest difference %.3g" % (burn, float(err.max())))
        assert (err > 2e-5).float().mean() <= 0.02, float(err.max())


def test_local_chains_sharded_over_chain_offset(ht):
    """The same global chains in two halves: a producer lane keys its Philox stream by chain_offset + chain."""
    C, N, L, burn, off = 48, 40, 25, 2, 1000
    t, th0 = _model(ht, 3, C, L)
    whole = _run(t, th0, N, L, burn, 1, off=off)
    h = C // 2
    lo = _run(t, th0[:h].contiguous(), N, L, burn, 1, off=off)
    hi = _run(t, th0[h:].contiguous(), N, L, burn, 1, off=off + h)
    _assert_same((torch.cat([lo[0], hi[0]], 1), torch.cat([lo[1], hi[1]]), torch.cat([lo[2], hi[2]])), whole, "sharded")
    _assert_same(whole, _run(t, th0, N, L, burn, 0, off=off), "whole")


@pytest.mark.parametrize("burn", [-1, 0, 3])
def test_local_repeats_params_init_when_every_proposal_diverges(ht, burn):
    """The step of tests/test_gpu_quad_rows.py::test_row_waves_repeat_params_init_when_every_proposal_diverges: every proposal is
    rejected, the row wave gets the sentinel only while the records keep flowing - every row equals params_init."""
    D, C, N, L = 3, 256, 40, 400
    rng = np.random.default_rng(5)
    Qm, _ = np.linalg.qr(rng.normal(size=(D, D)))
    P = (Qm * np.array([-0.5, 1.0, 2.0])) @ Qm.T
    t = _target(ht, 0.5 * (P + P.T), np.zeros(D))
    th0 = torch.tensor(0.1 * rng.normal(size=(C, D)), dtype=torch.float32, device=dev())
    samples, rej, fin = _run(t, th0, N, L, burn, 1, eps=2.0)
    rows = samples[1:N - burn]                       # the stored trajectories: burn + 1 ... N - 1
    assert torch.equal(rows, th0.cpu().expand_as(rows)), "a rejected trajectory must repeat the row bit for bit"
    assert torch.equal(rej, torch.full((C,), N, dtype=torch.int32))
    assert torch.equal(fin, th0.cpu())
    ref = _run(t, th0, N, L, burn, 0, eps=2.0)
    for x, y in zip((samples, rej, fin), ref):
        assert torch.equal(x, y)


def test_local_launch_against_the_oracle(ht):
    """D = 3, C = 256, N = 40, L = 25 against oracle/hmc_oracle.py in the band the suite holds fp32 Gaussian HMC to
    (tests/test_gpu_hmc.py::test_sample_fused_vs_oracle: 2e-4, at most 1 % of the chains on a borderline Metropolis decision;
    tests/test_gpu_quad_rows.py compares bit for bit and names no band of its own)."""
    import hmc_oracle as O
    from hamiltorch_amd import _abi
    C, D, N, L, burn, eps, seed = 256, 3, 40, 25, 3, 0.3, 11
    sigma = np.array([[1.0, 0.6, 0.2], [0.6, 2.0, 0.5], [0.2, 0.5, 0.5]])
    P = np.linalg.inv(sigma)
    t = _target(ht, P, np.zeros(D))
    th0 = (0.3 * O.philox_normals(seed, np.arange(C), 0, D, O.PURPOSE_INIT, dtype=np.float64)).astype(np.float32)
    samples, rej, fin = _run(t, torch.from_numpy(th0).to(dev()), N, L, burn, 1, eps=eps, seed=seed)
    assert _abi.get_tuning("quad_local") == 1
    assert _abi.last_route().startswith("hmc_gauss_quad_fused_kernel<3,25")
    ref, info = O.sample_hmc(O.GaussianTarget(np.zeros(D, np.float32), P.astype(np.float32), 0.0), th0, N, L, eps, burn, None,
                             O.PhiloxDraws(seed, np.arange(C)))
    ref = np.stack(ref)
    assert ref.shape[0] == N - burn                  # row 0 is params_init: the caller's, not the launch's
    got = samples[1:ref.shape[0]].numpy()
    err = np.abs(got - ref[1:]).max(axis=(0, 2))
    bad = err > 2e-4
    print("largest difference %.3g, %d of %d chains outside 2e-4" % (err.max(), bad.sum(), C))
    assert bad.mean() <= 0.01
    assert np.abs(fin.numpy() - ref[-1])[~bad].max() <= 2e-4
    want_rej = np.rint((1.0 - info["acc_rate"]) * N).astype(np.int64)
    np.testing.assert_array_equal(rej.numpy()[~bad], want_rej[~bad])
