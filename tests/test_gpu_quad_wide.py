"""GPU: tuning key "quad_wide" - the local quad launch with 16-byte LDS hand-overs per block of four trajectories
(csrc/hmc_gauss_quad_dev.hpp: hmc_gauss_quad_wide_kernel, quad_body WIDE) against the local launch with 4-byte hand-overs ("quad_wide" = 0,
hmc_gauss_quad_local_kernel).  Only the rings' addressing and the LDS instructions differ - same records, same arithmetic, same
groups and barriers - so samples, reject counts and the final state are equal BIT FOR BIT (torch.equal) and the status word is 0.
Shapes: the smallest at which a block of four positions can go wrong - every compiled instance, half a wave up to three blocks of
chains, every shape of the group sequence (a lead group plus one group of four, single trajectories after whole blocks, the Q2
single between blocks), launches chunked over `traj_offset`, and a run in which every proposal is rejected."""
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


def _run(t, th0, N, L, burn, wide, eps=0.3, seed=13, chunks=None):
    """(samples, reject counts, final state) of N trajectories through the C ABI on a prepared workspace, `chunks`: the trajectories
    per launch (one launch of N when absent); the status word must be 0"""
    from hamiltorch_amd import _abi
    C, D = th0.shape
    chunks = chunks or [N]
    assert sum(chunks) == N
    _abi.set_tuning("quad_rows", 1)
    _abi.set_tuning("quad_local", 1)
    _abi.set_tuning("quad_wide", wide)
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
        assert _abi.last_route().startswith("hmc_gauss_quad_fused_kernel<%d" % D), _abi.last_route()
        start += n
    # the route string is the same for both launches: the debug counter tells that the wide kernel, and only it, was launched
    assert _abi.get_tuning("quad_wide_launches") - launched == (len(chunks) if wide else 0)
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


def test_wide_is_the_default():
    from hamiltorch_amd import _abi
    assert _abi.get_tuning("quad_wide") == 1


# (N, burn): 8 = the lead group of 4 plus one group of 4; 9 = a single trajectory after whole blocks; 37 = 4 + 32 + 1 (L = 25; 4 + 16
# + 16 + 1 at the other L); 71 = 4 + 32 + 32 + 3 x 1; burn = 5: the burn-in phase is 4 + 1 + 1 and the Q2 trajectory opens the stored
# phase as a group of its own, between blocks; burn = 0: the Q2 single is first in its phase behind a burn-in phase of one;
# (40, 39): the Q2 single is the last trajectory of the launch
SEQUENCES = [(8, -1), (9, -1), (37, -1), (71, -1), (71, 5), (37, 0), (8, 5), (40, 39)]
# 8 chains are half a wave, 16 a full wave, 24 a partial second block, 40 three blocks (the fused route wants C % 8 == 0)
CHAINS = [8, 16, 24, 40]


# every compiled instance (L = 25: passes of 32; 10, 5: passes of 16) and the any-L one (7: passes of 16) at D = 1 ... 3, over every chain
# count, with the sequence that has every group size and the Q2 single between blocks
@pytest.mark.parametrize("L", [25, 10, 5, 7])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_wide_equals_local_over_instances_and_chain_counts(ht, D, L):
    for C in CHAINS:
        t, th0 = _model(ht, D, C, L)
        _assert_same(_run(t, th0, 71, L, 5, 1), _run(t, th0, 71, L, 5, 0), "D=%d L=%d C=%d" % (D, L, C))


# every shape of the group sequence on every instance, at the chain count with a partial block in the middle of the grid's tail
@pytest.mark.parametrize("N,burn", SEQUENCES)
@pytest.mark.parametrize("L", [25, 10, 5, 7])
def test_wide_group_sequences(ht, L, N, burn):
    for D, C in ((3, 40), (2, 24), (1, 8)):
        t, th0 = _model(ht, D, C, L)
        _assert_same(_run(t, th0, N, L, burn, 1), _run(t, th0, N, L, burn, 0), "D=%d L=%d C=%d N=%d burn=%d" % (D, L, C, N, burn))


@pytest.mark.parametrize("L,chunks", [(25, [41, 41]), (10, [8, 8, 8])])
def test_wide_launches_chunked_over_traj_offset(ht, L, chunks):
    """Every launch starts its own group sequence: positions count from the group's first trajectory, not from `traj_offset`."""
    t, th0 = _model(ht, 3, 40, L)
    N = sum(chunks)
    for burn in (-1, 12):
        _assert_same(_run(t, th0, N, L, burn, 1, chunks=chunks), _run(t, th0, N, L, burn, 0, chunks=chunks), "chunked, burn=%d" % burn)


@pytest.mark.parametrize("burn", [-1, 3])
def test_wide_repeats_params_init_when_every_proposal_diverges(ht, burn):
    """A step so large that every proposal diverges (tests/test_gpu_quad_local.py's): every message of every block is the sentinel,
    every row repeats params_init bit for bit and the reject count is N."""
    D, C, N, L = 3, 40, 40, 400
    rng = np.random.default_rng(5)
    Qm, _ = np.linalg.qr(rng.normal(size=(D, D)))
    P = (Qm * np.array([-0.5, 1.0, 2.0])) @ Qm.T
    t = _target(ht, 0.5 * (P + P.T), np.zeros(D))
    th0 = torch.tensor(0.1 * rng.normal(size=(C, D)), dtype=torch.float32, device=dev())
    samples, rej, fin = _run(t, th0, N, L, burn, 1, eps=2.0)
    # rows 1 ... N - 1 - burn are the stored trajectories burn + 1 ... N - 1; row 0 is the caller's and a row past them is nobody's:
    # the launch must leave both as they were (zero)
    last = N - 1 - burn
    rows = samples[1:last + 1]
    assert not samples[0].any() and not samples[last + 1:].any()
    assert torch.equal(rows, th0.cpu().expand_as(rows)), "a rejected trajectory must repeat the row bit for bit"
    assert torch.equal(rej, torch.full((C,), N, dtype=torch.int32))
    assert torch.equal(fin, th0.cpu())
    for x, y in zip((samples, rej, fin), _run(t, th0, N, L, burn, 0, eps=2.0)):
        assert torch.equal(x, y)
