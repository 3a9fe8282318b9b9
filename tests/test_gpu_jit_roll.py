"""GPU: likelihoods summed over data rows on the ROLLED callback route (hamiltorch_amd/jit/roll.py, csrc/jit/rolled_callback.hip.in)
against the torch-evaluated route of the same library (`native=False`: vmap(grad) per step + the pieces kernels) on the same Philox
streams.  Tolerances and exempt shares are those of tests/test_gpu_jit_split.py: compiled against torch in float64 1e-8 with 2 % of
the chains exempt (a chain whose accept decision flips on a last-bit difference), float32 2e-4 with 3 %.

The workgroup is 64 chains x W waves and the rows are divided over the waves: W = 1, 2 and 4 are forced through the engine's test
hook (`_CompiledRolledHMC.WAVES`); a fixed W gives the same bits from run to run (the partial sums are added in wave order),
different W agree at the tolerance (the order of the sum over rows differs).

The second half of the file compares the kernel with oracle/hmc_oracle.py:sample_hmc on the closed-form targets of jit_roll_cases.py -
nothing of the library on the reference side - chain by chain on the Philox draws of the same seed and chain offset, at the bounds of
tests/test_gpu_jit.py (float64 1e-9, float32 2e-4, 3 % of the chains exempt for a flipped accept, equal acceptance rates of the rest):
rows that do not divide over the waves, waves without rows, more waves than rows, two groups of unequal length, more than one tile
in the LDS form of the table reads, the three mass kinds, 1500-term sums and a run cut into launches at such a shape."""
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
    16 rows each, fewer than the tile of 85 and 64 rows: every wave stages ONE partly filled tile per group (a second tile:
    test_more_than_one_tile_in_the_lds_form) - at W = 1 and 4 against native=False, bit-identical run to run."""
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


# ---- against oracle.sample_hmc on the closed-form targets (jit_roll_cases.py) ------------------------------------------------------
TAG = {torch.float64: "f64", torch.float32: "f32"}
DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])


def tt(a, dtype):
    return None if a is None else torch.tensor(a, dtype=dtype, device="cuda")


def sample(ht, run, fn, dtype, **over):
    """sample() of a jit_roll_cases.Run -> (rows [n, C, D], acceptance rates [C])."""
    out, acc = ht.sample(fn, tt(run.start(dtype), dtype), inv_mass=tt(run.inv_mass(dtype), dtype), **dict(run.kwargs(), **over))
    assert len(out) == run.samples - max(run.burn, -1)
    return torch.stack(list(out)), acc


def against_oracle(got, acc, run, dtype, tol=None):
    """compare() of tests/test_gpu_jit.py: every chain within `tol` of the oracle's, at most 3 % exempt, and the acceptance rates of
    the others equal to the oracle's."""
    tol = cases.TOL[dtype] if tol is None else tol
    ref, info = run.oracle(dtype)
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == ref.dtype
    err = cases.deviation(got, ref)
    bad = ~(err <= tol)
    print("chains outside %.2e of the oracle: %d of %d; largest difference of the others %.3g; acceptance %.2f"
          % (tol, bad.sum(), bad.size, err[~bad].max() if (~bad).any() else np.nan, info["acc_rate"].mean()))
    assert bad.mean() <= cases.MAX_FLIPPED, "%d of %d chains differ (max err %.3g)" % (bad.sum(), bad.size, np.nanmax(err))
    np.testing.assert_allclose(acc.cpu().numpy()[~bad], info["acc_rate"][~bad], atol=1e-12)


def agree(a, b, dtype, tol=None):
    """Two runs of the kernel that sum the rows in another order: the same chains at the tolerance, 3 % exempt."""
    tol = cases.TOL[dtype] if tol is None else tol
    assert a.shape == b.shape
    err = (a - b).abs().amax(dim=(0, 2))
    assert float((~(err <= tol)).float().mean()) <= cases.MAX_FLIPPED, "max err %.3g" % float(err.max())


def min_rows(monkeypatch, rows):
    """roll.py forms a group from 8 rows (ROLL_MIN_ROWS).  The kernel takes any row count >= 1 per group, and its divisions of FEWER
    rows than that over the waves are reached by lowering the rule for the test."""
    from hamiltorch_amd.jit import roll
    if rows < roll.ROLL_MIN_ROWS:
        monkeypatch.setattr(roll, "ROLL_MIN_ROWS", rows)


def rolled_of(fn, th0, mass_kind=0):
    """The compiled program behind the last sample() of `fn` (the trace cache's entry): its roll.Rolled and the generated text."""
    from hamiltorch_amd import jit
    c = jit.compile_hmc(fn, th0[0], th0.dtype, mass_kind)
    assert isinstance(c, jit.CompiledRolled)
    return c.rolled, c.generated


def test_the_fewest_rows_a_group_is_formed_from():
    from hamiltorch_amd.jit import roll
    assert roll.ROLL_MIN_ROWS == 8 and (8, 8) in cases.EDGE_PAIRS[torch.float64] and (8, 16) in cases.EDGE_PAIRS[torch.float32]


@pytest.mark.parametrize("dtype,rows,W", [(d, r, w) for d in (torch.float64, torch.float32) for r, w in cases.EDGE_PAIRS[d]],
                         ids=lambda v: TAG.get(v, str(v)))
def test_rows_that_do_not_divide_over_the_waves(ht, dtype, rows, W, monkeypatch):
    """Logistic regression, D = 3, 130 chains, 10 trajectories of 5 steps.  Wave w takes rows [w per, min((w + 1) per, rows)), per =
    ceil(rows / W): (41, 4) and (17, 16) a short last wave, (13, 2) 7 + 6, (5, 4) 2 + 2 + 1 and a wave that starts AT rows, (9, 8) and
    (3, 8) waves that start BEYOND rows, (3, 8), (8, 16) and (9, 8) in float32 one row per wave and more waves than rows, (40, 16)
    3 rows per wave, the last wave 1 and two waves none; 8 rows is the fewest roll.py rolls.  Every pair against the oracle, bit-identical
    in a second run, and equal to W = 1 at the tolerance."""
    min_rows(monkeypatch, rows)
    run = cases.RUNS["rows%d" % rows]
    fn = run.fn(dtype, "cuda")
    waves(monkeypatch, W)
    got, acc = sample(ht, run, fn, dtype)
    assert "hta_cb_rolled_kernel<D=3,rows=%d,W=%d,%s,mass=0,U=0,groups=1," % (rows, W, TAG[dtype]) in route(), route()
    against_oracle(got, acc, run, dtype)
    again, acc2 = sample(ht, run, fn, dtype)
    assert torch.equal(again, got) and torch.equal(acc2, acc), "W = %d is not deterministic" % W
    waves(monkeypatch, 1)
    one, acc1 = sample(ht, run, fn, dtype)
    assert "rows=%d,W=1," % rows in route(), route()
    against_oracle(one, acc1, run, dtype)
    agree(got, one, dtype)


@pytest.mark.parametrize("table", ["direct", "lds"])
def test_two_groups_of_unequal_length(ht, table, monkeypatch):
    """Case 3 with 7 Poisson rows (3 slots) and 19 Gaussian rows (4 slots), float64.  W = 4: shares of 5, 5, 5, 4 and 2, 2, 2, 1.  W = 8:
    3 rows per wave leave wave 7 of the long group without rows (it starts beyond them) and wave 6 with one; 1 row per wave leaves
    wave 7 of the short group without (it starts at its end).  Both table forms."""
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_ROLL_TABLE", table)
    min_rows(monkeypatch, 7)
    run = cases.RUNS["two_structures"]
    fn = run.fn(torch.float64, "cuda")
    for W in (4, 8):
        waves(monkeypatch, W)
        got, acc = sample(ht, run, fn, torch.float64)
        assert "hta_cb_rolled_kernel<D=3,rows=19,W=%d,f64,mass=0,U=0,groups=2," % W in route(), route()
        against_oracle(got, acc, run, torch.float64)
        assert torch.equal(sample(ht, run, fn, torch.float64)[0], got)
    R, text = rolled_of(fn, tt(run.start(torch.float64), torch.float64))
    assert sorted(R.rows) == [7, 19] and "#define HTA_CB_TABLE_LDS %d" % (table == "lds") in text


@pytest.mark.parametrize("name,dtype,W", [("lds_logistic_1", torch.float64, 1), ("lds_logistic_1", torch.float32, 1),
                                          ("lds_logistic_2", torch.float64, 2), ("lds_hierarchical", torch.float64, 1)],
                         ids=lambda v: TAG.get(v, str(v)))
def test_more_than_one_tile_in_the_lds_form(ht, name, dtype, W, monkeypatch):
    """HAMILTORCH_AMD_JIT_ROLL_TABLE=lds with more rows per wave than a tile holds: the wave stages a second (and third) tile into
    the buffer it has just read the first from - the two wavefront fences and the wave barrier of the row loop order that.  Logistic
    D = 3 (3 slots, tile 85): 200 rows on one wave = 85 + 85 + 30, and 250 rows on two waves = 85 + 40 each; the hierarchical case
    (U = 1, 4 slots, tile 96): 300 rows on one wave = 96 + 96 + 96 + 12.  The tile is computed here from the compiled program, so that
    another tile formula cannot turn this back into a one-tile test unnoticed.  Against the oracle, against the direct form, bit-identical
    from run to run."""
    run = cases.RUNS[name]
    fn = run.fn(dtype, "cuda")
    waves(monkeypatch, W)
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_ROLL_TABLE", "lds")
    got, acc = sample(ht, run, fn, dtype)
    r = route()
    R, text = rolled_of(fn, tt(run.start(dtype), dtype))
    assert "#define HTA_CB_TABLE_LDS 1" in text and len(R.groups) == 1
    rows, slots = R.rows[0], R.groups[0].slots
    assert "hta_cb_rolled_kernel<D=%d,rows=%d,W=%d,%s,mass=0,U=%d,groups=1," % (run.D, rows, W, TAG[dtype], R.U) in r, r
    tile = (1 + run.D + R.U) * 64 // slots                         # rolled_callback.hip.in: rows per tile
    per = -(-rows // W)
    full, partial = divmod(min(per, rows - (W - 1) * per), tile)    # of the last wave (the others have `per` rows)
    assert tile < per and full >= (2 if W == 1 else 1) and partial > 0 and per % tile > 0, (tile, per, full, partial)
    against_oracle(got, acc, run, dtype)
    assert torch.equal(sample(ht, run, fn, dtype)[0], got)
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_ROLL_TABLE", "direct")
    direct, acc_d = sample(ht, run, fn, dtype)
    assert "#define HTA_CB_TABLE_LDS 0" in rolled_of(fn, tt(run.start(dtype), dtype))[1]
    against_oracle(direct, acc_d, run, dtype)
    agree(got, direct, dtype)


@DTYPES
@pytest.mark.parametrize("mass,burn", cases.MASS_ROWS)
def test_mass_matrices(ht, mass, burn, dtype, monkeypatch):
    """inv_mass None, (D,) and (D, D) - masses() of tests/test_gpu_jit.py - on the logistic case at W = 2, with burn = 0, 3 and -1: the
    momentum draw by the mass factor (the pre-drawn records), the drift and the kinetic energy in a block where wave 1 shadows wave 0."""
    run = cases.RUNS["mass_%s" % mass]
    assert run.burn == burn
    waves(monkeypatch, 2)
    got, acc = sample(ht, run, run.fn(dtype, "cuda"), dtype)
    assert "hta_cb_rolled_kernel<D=3,rows=40,W=2,%s,mass=%d," % (TAG[dtype], ["none", "diag", "full"].index(mass)) in route(), route()
    against_oracle(got, acc, run, dtype)


def test_full_mass_with_a_uniform(ht, monkeypatch):
    """The hierarchical case (the noise scale's node is a uniform: its adjoint comes back through the rest) under a full mass matrix,
    float64, W = 2, burn = 3."""
    run = cases.RUNS["mass_hierarchical"]
    waves(monkeypatch, 2)
    got, acc = sample(ht, run, run.fn(torch.float64, "cuda"), torch.float64)
    assert "hta_cb_rolled_kernel<D=4,rows=24,W=2,f64,mass=2,U=1,groups=1," in route(), route()
    against_oracle(got, acc, run, torch.float64)


# 1500-term sums in float32.  The band of the 40-row cases says nothing about them; the bound is derived on the CPU, never from the
# kernel: the oracle with the target evaluated in float32 against the oracle in float64 on the same start and draws (this run: 130
# chains, 8 trajectories of 5 steps at eps = 0.06, no accept decision differs) - the largest difference of a chain is
LONG_F32_MEASURED = 2.2e-7          # tests/test_jit_roll_cpu.py::test_the_float32_bound_of_the_long_sums measures it again (2.17e-7)
# and the kernel, which adds W partial sums in wave order where numpy adds pairwise, is allowed 4 times that:
LONG_F32_BOUND = 4 * LONG_F32_MEASURED


@pytest.mark.parametrize("dtype,W", [(torch.float32, 16), (torch.float32, 1), (torch.float64, 8)], ids=lambda v: TAG.get(v, str(v)))
def test_long_sums(ht, dtype, W, monkeypatch):
    """big_logistic, 1500 rows, D = 4, 130 chains, 8 trajectories of 5 steps at a step size that moves (the oracle accepts between 0.5
    and 1.0 of the proposals): float32 at W = 16 (94 rows per wave, the last 90) and W = 1 within LONG_F32_BOUND of the float32
    oracle, float64 at W = 8 (188 rows per wave, the last 184) within 1e-9.  (W = 1 is what made the kernel sum its rows in blocks of
    64: with one accumulator over the 1500 rows it was 1.16e-6 from the oracle, 7 of the 130 chains outside the bound; in blocks it
    is 3.2e-7, and 2.8e-7 at W = 16.)"""
    run = cases.RUNS["long"]
    assert 0.5 <= run.oracle(dtype)[1]["acc_rate"].mean() <= 1.0
    waves(monkeypatch, W)
    got, acc = sample(ht, run, run.fn(dtype, "cuda"), dtype)
    assert "hta_cb_rolled_kernel<D=4,rows=1500,W=%d,%s,mass=0,U=0,groups=1," % (W, TAG[dtype]) in route(), route()
    against_oracle(got, acc, run, dtype, LONG_F32_BOUND if dtype == torch.float32 else None)


def test_an_edge_shape_cut_into_launches_is_bit_identical(ht, monkeypatch):
    """41 rows over 4 waves (11, 11, 11, 8) with a diagonal mass matrix, 12 trajectories, burn = 2: verbose progress cuts the run into
    launches; the same bits as the single launch, which agrees with the oracle."""
    run = cases.RUNS["chunks"]
    fn = run.fn(torch.float64, "cuda")
    waves(monkeypatch, 4)
    one, acc = sample(ht, run, fn, torch.float64)
    assert "hta_cb_rolled_kernel<D=3,rows=41,W=4,f64,mass=1," in route(), route()
    against_oracle(one, acc, run, torch.float64)
    many, acc_many = sample(ht, run, fn, torch.float64, verbose=True)
    assert "hta_cb_rolled_kernel<D=3,rows=41,W=4,f64,mass=1," in route() and torch.equal(one, many) and torch.equal(acc, acc_many)
