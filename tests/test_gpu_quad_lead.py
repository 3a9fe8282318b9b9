"""GPU: tuning keys "quad_rows_wt" (the row wave of the local and wide launches stores the sample rows write-through at agent scope)
and "quad_lead" (the wide launch with 512 threads: waves 4-7 draw records up to the launch's first full pass;
csrc/hmc_gauss_quad_dev.hpp: hmc_gauss_quad_lead_kernel, quad_local_produce LEAD, quad_rows_body WT).  Neither changes what is computed or
where it is stored - the same records in the same LDS slots, the same row values at the same addresses - so with both keys on
(1) the samples, the reject counts and the final state equal, BIT FOR BIT (torch.equal), those with both keys off (0: the
256-thread launch with plain row stores) and those with "quad_wide" = 0 (the local launch, its rows written through: the other
launch "quad_rows_wt" applies to); the status word is 0.

Chain counts.  1, 15, 16, 17 and 33 sit around the block edge of 16 chains.  The dispatcher takes the one-launch route only for
C % 8 == 0 (rows of whole 128-byte lines; tests/test_gpu_hmc.py::test_fused_quad_launch_needs_a_prepared_workspace_and_whole_lines
holds that), so of these only 16 reaches the kernels the keys act on; at the others the keys must change nothing either, and the
route and the launch counter say which launch ran.  8 (half a block), 24 (a block whose trailing chains lie past a.C) and 40
(three blocks, the last one half past a.C) are the block edges that do reach them.

Group sequences (quad_local_groups; a pass is 32 trajectories at L = 25 and 16 at L = 5 and the any-L instance, L = 7): the lead
group of 4, full passes, groups of 4, single ones.  n_traj = 8, 9, 35, 36, 37, 40, 41 sit below, at and across every boundary of
4 + 32 + 4; burn = -1 has no burn-in phase, burn = 1 puts trajectory burn + 1 (the Q2 instance, a group of its own) where the lead
group would be (the launch then has no lead group: 1 + 1 + Q2 + passes), burn = 3 puts it behind the lead group, at the position
where the first full pass would start."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ON = dict(quad_wide=1, quad_rows_wt=1, quad_lead=1)
OFF = dict(quad_wide=1, quad_rows_wt=0, quad_lead=0)
LOCAL = dict(quad_wide=0, quad_rows_wt=1, quad_lead=1)       # ("quad_lead" does not apply to the local launch)


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


def _run(t, th0, N, L, burn, keys, eps=0.3, seed=13, chunks=None):
    """(samples, reject counts, final state) of N trajectories through the C ABI on a prepared workspace, `chunks`: the trajectories
    per launch (one launch of N when absent; equal ones: a workspace is prepared for one launch length).  Asserts the route, the launch counter and a zero status word."""
    from hamiltorch_amd import _abi
    C, D = th0.shape
    chunks = chunks or [N]
    assert sum(chunks) == N
    _abi.set_tuning("quad_rows", 1)
    _abi.set_tuning("quad_local", 1)
    for k, v in keys.items():
        _abi.set_tuning(k, v)
    one_launch = C % 8 == 0
    ws = torch.zeros(_abi.gaussian_workspace_bytes(C, D, max(chunks), 4), dtype=torch.uint8, device=dev())
    _abi.hmc_gaussian_prepare(th0, t.precision, 0, None, C, D, max(chunks), ws)
    nrow = N - max(burn, 0) + 1
    samples = torch.zeros(nrow, C, D, device=dev())
    rej = torch.zeros(C, dtype=torch.int32, device=dev())
    cur = th0.clone()
    start = 0
    launched = _abi.get_tuning("quad_wide_launches")
    for n in chunks:
        _abi.hmc_gaussian_sample(cur, th0, t.precision, t.mean, t.log_norm, 0, None, None, L, eps, n, start, burn, seed, 0, samples, rej,
                                 workspace=ws)
        want = "hmc_gauss_quad_fused_kernel<%d" % D if one_launch else "hmc_gauss_quad_kernel<%d" % D
        assert _abi.last_route().startswith(want), (C, _abi.last_route())
        start += n
    # the route string is the same for the local, the wide and the 512-thread launch: the counter tells that a wide one was launched
    assert _abi.get_tuning("quad_wide_launches") - launched == (len(chunks) if keys["quad_wide"] and one_launch else 0)
    torch.cuda.synchronize()
    if one_launch:
        word = _abi.hmc_gaussian_status_word(ws, C, D, max(chunks), 4)
        assert word is not None and int(word) == 0
    _abi.hmc_gaussian_forget(ws)
    return samples.cpu(), rej.cpu(), cur.cpu()


def _assert_same(a, b, what):
    for x, y, name in zip(a, b, ("samples", "reject counts", "final state")):
        assert torch.equal(x, y), "%s: %s differ" % (what, name)
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[2]).all()


def _three_ways(t, th0, N, L, burn, what, **kw):
    on = _run(t, th0, N, L, burn, ON, **kw)
    _assert_same(on, _run(t, th0, N, L, burn, OFF, **kw), what + " (both keys off)")
    _assert_same(on, _run(t, th0, N, L, burn, LOCAL, **kw), what + " (quad_wide = 0)")
    return on


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


def test_the_keys_exist_and_reset_to_their_defaults():
    from hamiltorch_amd import _abi
    dflt = {k: _abi.get_tuning(k) for k in ("quad_rows_wt", "quad_lead")}
    assert set(dflt.values()) <= {0, 1}
    for k in dflt:
        _abi.set_tuning(k, 1 - dflt[k])
    _abi.reset_tuning()
    assert {k: _abi.get_tuning(k) for k in dflt} == dflt


CHAINS = [1, 15, 16, 17, 33, 8, 24, 40]
LS = [25, 5, 7]
N_TRAJ = [8, 9, 35, 36, 37, 40, 41]
BURNS = [-1, 1, 3]


# every chain count on every instance (D = 1 ... 3; L = 25, L = 5 and the any-L instance), with the sequence that has a burn-in phase
# that is the lead group, the Q2 single at the first position of the full pass, a full pass (two at the other L) and groups behind it
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("D", [1, 2, 3])
def test_keys_change_no_byte_over_chain_counts_and_instances(ht, D, L):
    for C in CHAINS:
        t, th0 = _model(ht, D, C, L)
        _three_ways(t, th0, 41, L, 3, "D=%d L=%d C=%d" % (D, L, C))


# every launch length against every place of the Q2 trajectory, on every pass length, at the chain count whose last block is half
# past a.C (and at the block edge itself)
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("burn", BURNS)
def test_keys_change_no_byte_over_group_sequences(ht, L, burn):
    for N in N_TRAJ:
        for D, C in ((3, 40), (2, 16)):
            t, th0 = _model(ht, D, C, L)
            _three_ways(t, th0, N, L, burn, "D=%d L=%d C=%d N=%d burn=%d" % (D, L, C, N, burn))


@pytest.mark.parametrize("L", [25, 7])
def test_two_consecutive_calls_equal_one_call_of_the_sum(ht, L):
    """`traj_offset` continued: the second launch starts a group sequence of its own (a lead-in of its own, all six producer waves
    again).  The two calls are the same bytes under all three key settings.  Against ONE call of the sum the eigenbasis route
    promises equality to rounding only, with the keys or without: the chain crosses a launch boundary as q = mu + Q y and comes
    back as y = Q^T (q - mu).  The band is the one tests/test_gpu_hmc.py::test_chunked_launches_equal_single_launch holds that
    property to: 2e-5, on all but 2 % of the chains (a borderline Metropolis decision); 256 chains, so that 2 % is more than none."""
    t, th0 = _model(ht, 3, 256, L)
    for burn in (-1, 3, 38):          # (38: the Q2 trajectory is the first of the second call, in its lead-in)
        one = _run(t, th0, 78, L, burn, ON)
        two = _three_ways(t, th0, 78, L, burn, "two calls, burn=%d" % burn, chunks=[39, 39])
        assert one[0].shape == two[0].shape
        for x, y in ((one[0], two[0]), (one[2][None], two[2][None])):
            err = (x - y).abs().amax(dim=(0, 2))
            print("L=%d burn=%d: max |two calls - one call| = %.3g, chains over 2e-5: %d" % (L, burn, float(err.max()), int((err > 2e-5).sum())))
            assert (err > 2e-5).float().mean() <= 0.02, float(err.max())
        assert (one[1] != two[1]).float().mean() <= 0.02


def test_both_metropolis_branches(ht):
    """A step large enough that proposals are accepted AND rejected: the sentinel and the accepted y both travel through the
    hand-over.  eps is chosen on the CPU oracle (oracle/hmc_oracle.py): the largest candidate whose oracle acceptance lies in
    [0.2, 0.8]; on the GPU the acceptance must then lie strictly between 0 and 1, chain by chain summed and in total."""
    import hmc_oracle as O
    D, C, N, L, burn, seed = 3, 40, 41, 25, 3, 13
    P = rand_spd(D, 8 + D)
    rng = np.random.default_rng(3)
    th0 = rng.normal(size=(C, D)).astype(np.float32)
    eps = None
    for cand in (1.38, 1.3, 1.2, 1.0):          # (largest frequency sqrt(2): the integrator is stable below eps = 1.414)
        _, info = O.sample_hmc(O.GaussianTarget(np.zeros(D, np.float32), P.astype(np.float32), 0.0), th0, N, L, cand, burn, None,
                               O.PhiloxDraws(seed, np.arange(C)))
        acc = float(np.mean(info["acc_rate"]))
        print("oracle: eps %.2f acceptance %.3f" % (cand, acc))
        if 0.2 <= acc <= 0.8:
            eps = cand
            break
    assert eps is not None
    t = _target(ht, P, np.zeros(D))
    samples, rej, fin = _three_ways(t, torch.from_numpy(th0).to(dev()), N, L, burn, "eps=%.2f" % eps, eps=eps, seed=seed)
    acc = 1.0 - float(rej.sum()) / (N * C)
    print("GPU: eps %.2f acceptance %.3f" % (eps, acc))
    assert 0.0 < acc < 1.0
    assert 0 < int(rej.sum()) < N * C
