"""GPU: tuning key "quad_rows" - the fused quad launch with the sample rows on row waves (csrc/hmc_gauss_quad_dev.hpp: ROWS; the
integrating wave hands every trajectory's outcome over through an LDS ring) against the same launch with every consumer wave
storing its own rows ("quad_rows" = 0).  The row wave rebuilds the row element from the accepted eigen-coordinate with the
instructions the integrating wave used, so samples, reject counts and the final state are equal BIT FOR BIT (torch.equal), over
repeated launches on one workspace."""
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


def _both(ht, t, th0, C, D, N, L, burn, eps=0.3, reps=4):
    """{rows: (samples and reject counts of `reps` launches on one workspace, final state)}; the state travels from launch to launch"""
    from hamiltorch_amd import _abi
    nbytes = _abi.gaussian_workspace_bytes(C, D, N, 4)
    outs = {}
    for rows in (0, 1):
        _abi.set_tuning("quad_rows", rows)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev())
        _abi.hmc_gaussian_prepare(th0, t.precision, 0, None, C, D, N, ws)
        res = []
        cur = th0.clone()
        for rep in range(reps):
            nrow = N - max(burn, 0) + 1
            samples = torch.zeros(nrow, C, D, device=dev()); rej = torch.zeros(C, dtype=torch.int32, device=dev())
            _abi.hmc_gaussian_sample(cur, th0, t.precision, t.mean, t.log_norm, 0, None, None, L, eps, N, 0, burn, 13 + rep, 0, samples, rej,
                                     workspace=ws)
            route = _abi.last_route()
            res.append(torch.cat([samples.reshape(-1), rej.float()]))
        torch.cuda.synchronize()
        assert route.startswith("hmc_gauss_quad_fused_kernel<%d" % D), route
        word = _abi.hmc_gaussian_status_word(ws, C, D, N, 4)
        assert word is not None and int(word) == 0
        outs[rows] = (torch.cat(res).cpu(), cur.cpu())
        _abi.hmc_gaussian_forget(ws)
    return outs


def _assert_equal(outs):
    assert torch.equal(outs[0][0], outs[1][0]), "samples / reject counts differ"
    assert torch.equal(outs[0][1], outs[1][1]), "final state differs"
    assert torch.isfinite(outs[1][0]).all() and torch.isfinite(outs[1][1]).all()


def _case(ht, D, C, N, L, burn):
    rng = np.random.default_rng(100 * D + L)
    mu = rng.normal(size=D)
    t = _target(ht, rand_spd(D, 8 + D), mu)
    th0 = torch.tensor(mu + rng.normal(size=(C, D)), dtype=torch.float32, device=dev())
    _assert_equal(_both(ht, t, th0, C, D, N, L, burn))


# the parameter list of tests/test_gpu_hmc.py::test_fused_quad_launch_is_bit_identical
@pytest.mark.parametrize("D,C,N,L,burn", [(3, 1024, 1000, 25, -1), (3, 1024, 200, 25, 20), (2, 512, 333, 10, 5), (4, 264, 97, 5, -1),
                                          (1, 64, 40, 7, 3), (3, 4096, 120, 25, -1)])
def test_row_waves_are_bit_identical_on_the_fused_launch_cases(ht, D, C, N, L, burn):
    _case(ht, D, C, N, L, burn)


# chain counts that leave a partial last wave (16 chains per wave) and a partial last block - one whose second integrating wave has
# no chain at all included (40 = 2.5 waves); the fused launch needs rows of whole 128-byte lines: C % 8 == 0 at D <= 3
@pytest.mark.parametrize("C", [8, 40, 264, 1000])
def test_row_waves_with_partial_waves_and_blocks(ht, C):
    _case(ht, 3, C, 75, 25, 4)


# trajectory counts that end in each tail loop: the pass of the unrolled loop is 32 trajectories at L = 25 and 16 otherwise, the
# tail pass 4, then single trajectories; with every place of the Q2 trajectory (burn = n_traj - 1: first and only stored one)
@pytest.mark.parametrize("L", [25, 10])
@pytest.mark.parametrize("N", [64, 36, 39, 8])
@pytest.mark.parametrize("burn", [-1, 0, 5, "last"])
def test_row_waves_tail_loops_and_burn(ht, L, N, burn):
    _case(ht, 3, 256, N, L, N - 1 if burn == "last" else burn)


@pytest.mark.parametrize("burn", [-1, 0, 3])
def test_row_waves_repeat_params_init_when_every_proposal_diverges(ht, burn):
    """A large step on an indefinite precision: every trajectory overflows, every proposal is rejected - the row wave gets the
    sentinel only, so every stored row and the final state repeat params_init bit for bit and every trajectory counts as rejected."""
    from hamiltorch_amd import _abi
    D, C, N, L = 3, 256, 40, 400
    rng = np.random.default_rng(5)
    Qm, _ = np.linalg.qr(rng.normal(size=(D, D)))
    P = (Qm * np.array([-0.5, 1.0, 2.0])) @ Qm.T
    t = _target(ht, 0.5 * (P + P.T), np.zeros(D))
    th0 = torch.tensor(0.1 * rng.normal(size=(C, D)), dtype=torch.float32, device=dev())
    outs = _both(ht, t, th0, C, D, N, L, burn, eps=2.0, reps=2)
    _assert_equal(outs)
    nrow = N - max(burn, 0) + 1
    per = nrow * C * D + C
    for rep in range(2):
        blk = outs[1][0][rep * per:(rep + 1) * per]
        rows = blk[:nrow * C * D].reshape(nrow, C, D)[1:N - burn]      # the stored trajectories: burn + 1 ... N - 1
        assert torch.equal(rows, th0.cpu().expand_as(rows)), "a rejected trajectory must repeat the row bit for bit"
        assert torch.equal(blk[nrow * C * D:], torch.full((C,), float(N)))
    assert torch.equal(outs[1][1], th0.cpu())
    assert _abi.last_route().startswith("hmc_gauss_quad_fused_kernel<3")
