"""GPU: likelihoods summed over data rows on the ROLLED callback route (hamiltorch_amd/jit/roll.py, csrc/jit/rolled_callback.hip.in)
against the torch-evaluated route of the same library (`native=False`: vmap(grad) per step + the pieces kernels) on the same Philox
streams.  Tolerances and exempt shares are those of tests/test_gpu_jit_split.py: compiled against torch in float64 1e-8 with 2 % of
the chains exempt (a chain whose accept decision flips on a last-bit difference), float32 2e-4 with 3 %.

The workgroup is 64 chains x W waves and the rows are divided over the waves: W = 1, 2 and 4 are forced through the engine's test
hook (`_CompiledRolledHMC.WAVES`); a fixed W gives the same bits from run to run (the partial sums are added in wave order),
different W agree at the tolerance (the order of the sum over rows differs)."""
import numpy as np
import pytest
import torch

import jit_roll_cases as cases

pytestmark = pytest.mark.gpu

TOL = {torch.float64: (1e-8, 0.02), torch.float32: (2e-4, 0.03)}


@pytest.fixture(scope="module")
def ht():
    import hamiltorch_amd
    assert torch.cuda.is_available()
    return hamiltorch_amd


@pytest.fixture(autouse=True)
def forced(monkeypatch):
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_ROLL", "force")


def route():
    from hamiltorch_amd import _abi
    return _abi.last_route()


def start(C, D, dtype, seed=5, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(C, D, generator=g, dtype=torch.float64)).to(dtype).cuda()


def run(ht, fn, th0, **kw):
    kw = dict(dict(num_samples=10, num_steps_per_sample=5, step_size=0.08, verbose=False, seed=11), **kw)
    return torch.stack(list(ht.sample(fn, th0, **kw)))


def waves(monkeypatch, W):
    from hamiltorch_amd import samplers
    monkeypatch.setattr(samplers._CompiledRolledHMC, "WAVES", W)


def close(a, b, dtype):
    tol, share = TOL[dtype]
    assert a.shape == b.shape
    err = (a - b).abs().amax(dim=(0, 2))
    bad = ~(err <= tol)
    print("chains outside %.1e: %d of %d (largest difference %.3g)" % (tol, int(bad.sum()), bad.numel(), float(err.max())))
    assert float(bad.float().mean()) <= share, "%d of %d chains differ (max err %.3g)" % (int(bad.sum()), bad.numel(), float(err.max()))


_ref = {}


def reference(ht, name, fn, th0, **kw):
    """The torch-evaluated run of a case: computed once, shared, left unchanged."""
    if name not in _ref:
        _ref[name] = run(ht, fn, th0, native=False, **kw)
        assert "hta_cb_rolled_kernel" not in route() and "native=False" in route(), route()
    return _ref[name]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_logistic_rows_over_1_2_4_waves(ht, dtype, monkeypatch):
    """Case 1, C = 130 (a partial last wave of chains): every W against native=False; W = 2 and W = 4 bit-identical run to run;
    W = 2 and W = 4 against W = 1 at the same tolerance."""
    fn = cases.logistic(dtype=dtype, device="cuda")
    th0 = start(130, 3, dtype)
    ref = reference(ht, "logistic-%s" % dtype, fn, th0)
    got = {}
    for W in (1, 2, 4):
        waves(monkeypatch, W)
        got[W] = run(ht, fn, th0)
        assert "hta_cb_rolled_kernel<D=3,rows=40,W=%d,%s" % (W, "f64" if dtype == torch.float64 else "f32") in route(), route()
        close(got[W], ref, dtype)
        if W > 1:
            assert torch.equal(run(ht, fn, th0), got[W]), "W = %d is not deterministic" % W
            close(got[W], got[1], dtype)


@pytest.mark.parametrize("case", ["hierarchical", "two_structures"])
def test_uniforms_and_two_groups(ht, case, monkeypatch):
    """Case 2 (the noise scale's nodes are uniforms: their adjoints come back through the rest) and case 3 (two groups + a rest),
    float64, W = 2."""
    fn = getattr(cases, case)(device="cuda")
    D = 4 if case == "hierarchical" else 3
    th0 = start(96, D, torch.float64, scale=0.2)
    kw = dict(step_size=0.03)
    ref = reference(ht, case, fn, th0, **kw)
    waves(monkeypatch, 2)
    got = run(ht, fn, th0, **kw)
    r = route()
    if case == "hierarchical":
        assert "hta_cb_rolled_kernel<D=4,rows=24,W=2,f64" in r and "groups=1" in r and "U=0" not in r, r
    else:
        assert "hta_cb_rolled_kernel<D=3,rows=16,W=2,f64" in r and "groups=2" in r, r
    close(got, ref, torch.float64)


def test_the_lds_form_of_the_table_reads(ht, monkeypatch):
    """HAMILTORCH_AMD_JIT_ROLL_TABLE=lds (a tile of rows per wave staged through LDS) on case 3 - two groups of different slot counts,
    rows that do not fill the last tile - at W = 1 and 4 against native=False, bit-identical run to run."""
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_ROLL_TABLE", "lds")
    fn = cases.two_structures(device="cuda")
    th0 = start(96, 3, torch.float64, scale=0.2)
    ref = reference(ht, "two_structures", fn, th0, step_size=0.03)
    for W in (1, 4):
        waves(monkeypatch, W)
        got = run(ht, fn, th0, step_size=0.03)
        assert "hta_cb_rolled_kernel<D=3,rows=16,W=%d,f64" % W in route(), route()
        close(got, ref, torch.float64)
        assert torch.equal(run(ht, fn, th0, step_size=0.03), got)


def test_no_leapfrog_steps(ht, monkeypatch):
    """L = 0: no gradient call, hence no barrier of its own, between the first evaluation and a rejection in the same trajectory;
    every proposal equals the current state, so every row of the run is the start."""
    fn = cases.logistic(device="cuda")
    th0 = start(70, 3, torch.float64)
    waves(monkeypatch, 4)
    got = run(ht, fn, th0, num_steps_per_sample=0, num_samples=6)
    assert "hta_cb_rolled_kernel" in route(), route()
    assert torch.equal(got, th0[None].expand_as(got))


@pytest.mark.parametrize("burn", [0, 3, -1])
def test_burn_in(ht, burn, monkeypatch):
    fn = cases.logistic(device="cuda")
    th0 = start(70, 3, torch.float64)
    waves(monkeypatch, 2)
    got = run(ht, fn, th0, burn=burn)
    assert "hta_cb_rolled_kernel" in route(), route()
    close(got, run(ht, fn, th0, burn=burn, native=False), torch.float64)


def test_a_run_cut_into_launches_is_bit_identical(ht, monkeypatch):
    """verbose progress cuts the run into launches that resume from the carried (log p, gradient) pair in the workspace."""
    fn = cases.logistic(device="cuda")
    th0 = start(70, 3, torch.float64)
    waves(monkeypatch, 4)
    kw = dict(num_samples=12, burn=2)
    one = run(ht, fn, th0, **kw)
    many = run(ht, fn, th0, **dict(kw, verbose=True))
    assert "hta_cb_rolled_kernel" in route() and torch.equal(one, many)


def test_nuts_adapts_the_same_step_size(ht, monkeypatch):
    fn = cases.logistic(device="cuda")
    th0 = start(64, 3, torch.float64)
    waves(monkeypatch, 2)
    kw = dict(num_samples=10, num_steps_per_sample=5, step_size=0.08, burn=4, sampler=ht.Sampler.HMC_NUTS, debug=2, verbose=False, seed=11)
    _, eps_a = ht.sample(fn, th0, **kw)
    assert "hta_cb_rolled_kernel" in route(), route()
    _, eps_b = ht.sample(fn, th0, native=False, **kw)
    assert abs(eps_a - eps_b) <= 1e-6 * abs(eps_b), (eps_a, eps_b)


def test_divergent_chains_are_rejected(ht, monkeypatch):
    """A step size far too large: non-finite energies reject (S:1045-1057), nothing traps, the samples stay finite; the same chains at
    a sane step size afterwards are unaffected."""
    fn = cases.logistic(dtype=torch.float32, device="cuda")
    th0 = start(96, 3, torch.float32)
    waves(monkeypatch, 2)
    out, acc = ht.sample(fn, th0, num_samples=8, num_steps_per_sample=6, step_size=40.0, debug=2, verbose=False, seed=3)
    assert "hta_cb_rolled_kernel" in route(), route()
    s = torch.stack(list(out))
    assert torch.isfinite(s).all() and float(acc.mean()) < 0.2
    close(run(ht, fn, th0), run(ht, fn, th0, native=False), torch.float32)


def test_auto_rolls_what_straight_line_code_refuses(ht, monkeypatch):
    """N = 1500 rows, D = 4: refused for its size before (the torch-evaluated route), rolled now; verify() passed (no fallback)."""
    import warnings
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_ROLL", "auto")
    fn = cases.big_logistic(device="cuda")
    th0 = start(64, 4, torch.float64, scale=0.1)
    kw = dict(num_samples=3, num_steps_per_sample=2, step_size=0.01)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = run(ht, fn, th0, **kw)
    r = route()
    assert "hta_cb_rolled_kernel<D=4,rows=1500," in r and "not compiled" not in r, r
    close(got, run(ht, fn, th0, native=False, **kw), torch.float64)


def test_stale_traces(ht, monkeypatch):
    """Data changed IN PLACE under a reused trace: verify() notices, one re-trace, the right result.  Data REPLACED by same-shape
    data (a new closure): the code object and the loaded module are reused, the tables are new, the right result."""
    from hamiltorch_amd import jit
    fn = cases.logistic(device="cuda")
    th0 = start(64, 3, torch.float64)
    waves(monkeypatch, 2)
    run(ht, fn, th0)
    traced = jit.stats["traced"]
    fn.data[0].mul_(-1.5)                                   # X: every slot of the table changes (the version counter moves)
    got = run(ht, fn, th0)
    assert jit.stats["traced"] == traced + 1 and "hta_cb_rolled_kernel" in route(), route()
    close(got, run(ht, fn, th0, native=False), torch.float64)
    with torch.no_grad():
        fn.data[0].data.copy_(fn.data[0].data * 0.5)        # behind the version counter: the trace is reused, the check catches it
    got = run(ht, fn, th0)
    assert "hta_cb_rolled_kernel" in route(), route()
    close(got, run(ht, fn, th0, native=False), torch.float64)
    other = cases.logistic(device="cuda", seed=9)
    compiled, loaded = jit.runtime.stats["compiled"], jit.runtime.stats["loaded"]
    got = run(ht, other, th0)
    assert jit.runtime.stats["compiled"] == compiled and jit.runtime.stats["loaded"] == loaded and "hta_cb_rolled_kernel" in route()
    close(got, run(ht, other, th0, native=False), torch.float64)
