"""CPU: the rolling pass of the callback compiler (hamiltorch_amd/jit/roll.py) up to and including the gfx950 code object of the
rolled trajectory kernel (csrc/jit/rolled_callback.hip.in) - no GPU needed.

* likelihoods summed over data rows roll into groups (one term function + a table of per-row constants), shared nodes become
  uniforms, what does not repeat stays in the rest; the rolled program's numpy interpreter reproduces torch.autograd in float64;
* the generated text holds no data: another data set of the same structure gives the same text (the module cache key);
* HAMILTORCH_AMD_JIT_ROLL=auto leaves every callable that compiled before on its straight-line text and rolls what was refused
  for its size; the refusals name their numbers; lists, leapfrog paths and the derivative kernels refuse a rolled-only callable;
* hipRTC builds the kernel for gfx950 in float32 and float64, the info block is as specified, float32 uses no scratch;
* hta_jit_rolled_sample turns bad arguments down before it looks at a device;
* the oracle targets of tests/jit_roll_cases.py (closed-form numpy, what the GPU tests hand to oracle.sample_hmc) against
  torch.autograd of their callables, and the float32 oracle against the float64 oracle on every float32 run of the GPU tests.
"""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import jit_roll_cases as cases
from hamiltorch_amd import _abi, jit
from hamiltorch_amd.jit import emit, roll, runtime
from hamiltorch_amd.jit.ir import Unsupported
from hamiltorch_amd.jit.trace import trace_callback

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
f64 = torch.float64


def rolled(fn, D):
    tr = trace_callback(fn, torch.full((D,), 0.2, dtype=f64))
    return tr, runtime.rolled_program(tr)


def against_autograd(fn, R, D, points=12, rtol=1e-10):
    pts = 0.5 * np.random.default_rng(7).standard_normal((points, D))
    mine = R.evaluate(pts, np.float64)
    for k in range(points):
        x = torch.tensor(pts[k], dtype=f64, requires_grad=True)
        v = fn(x)
        g, = torch.autograd.grad(v, x)
        ref = np.concatenate([[float(v.detach())], g.numpy()])
        assert np.all(np.abs(mine[k] - ref) <= rtol * (1.0 + np.abs(ref))), (k, mine[k], ref)


def test_logistic_regression_rolls_into_one_group():
    fn = cases.logistic()
    tr, R = rolled(fn, 3)
    assert R.rows == [40] and R.U == 0 and R.groups[0].slots == 3          # 40 rows, the three features; labels became signs
    assert R.groups[0].template.n_inputs == 3 + 0 + 3
    # the rest holds the prior: it depends on every weight, and on nothing else
    assert R.rest.evaluate([R.rest_value], np.array([[1.0, 2.0, 3.0]]))[0, 0] == pytest.approx(-7.0)
    against_autograd(fn, R, 3)


def test_hierarchical_scale_becomes_a_uniform():
    fn = cases.hierarchical()
    tr, R = rolled(fn, 4)
    assert R.rows == [24] and R.U >= 1
    for n in R.u_nodes:                                                    # the uniforms are functions of th[3] alone
        ins = {R.rest.nodes[i][1] for i in R.rest.reachable([n]) if R.rest.nodes[i][0] == "in"}
        assert ins == {3}, ins
    against_autograd(fn, R, 4)                                             # incl. d / d th[3]: the adjoint path through gu
    pts = 0.3 * np.random.default_rng(1).standard_normal((12, 4))
    g3 = R.evaluate(pts, np.float64)[:, 4]
    for k in range(12):
        x = torch.tensor(pts[k], dtype=f64, requires_grad=True)
        ref = float(torch.autograd.grad(fn(x), x)[0][3])
        assert abs(g3[k] - ref) <= 1e-10 * (1.0 + abs(ref))


def test_two_structures_and_a_row_that_folds():
    fn = cases.two_structures()
    tr, R = rolled(fn, 3)
    assert sorted(R.rows) == [16, 16] and len(R.groups) == 2              # 16 Poisson rows (of 17: the x = 0 row folded to a constant), 16 Gaussian
    assert R.rest_live > 0
    against_autograd(fn, R, 3)


def test_same_structure_other_data_same_text():
    a, b = cases.logistic(seed=0), cases.logistic(seed=5)
    (_, Ra), (_, Rb) = rolled(a, 3), rolled(b, 3)
    for dtype in (torch.float32, f64):
        ta, tb = runtime.rolled_generated_source(Ra, dtype, 0), runtime.rolled_generated_source(Rb, dtype, 0)
        assert ta == tb
        assert "term_0" in ta and "HTA_CB_SLOTS_0 3" in ta and "HTA_CB_GROUPS 1" in ta and "HTA_CB_U 0" in ta
    assert Ra.groups[0].table.shape == Rb.groups[0].table.shape == (40, 3) and not np.allclose(Ra.groups[0].table, Rb.groups[0].table)
    X = a.data[0].numpy() * np.where(a.data[1].numpy() > 0.5, 1.0, -1.0)[:, None]       # the labels as signs of the rows
    rows_of = lambda M: sorted(tuple(sorted(r)) for r in np.round(M, 12))                # (the slots are in first-visit order of the row's sum)
    assert rows_of(Ra.groups[0].table) == rows_of(X)
    assert not any(repr(float(v))[:8] in ta for v in a.data[0].flatten()[:20])          # no data literal in the text


def test_auto_keeps_what_compiled_and_rolls_what_was_refused(monkeypatch):
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_ROLL", "auto")
    small = cases.logistic(N=12, D=3, seed=4)
    ex = torch.full((3,), 0.2, dtype=f64)
    c = jit.compile_hmc(small, ex, f64, 0)
    assert type(c) is jit.CompiledHMC and c.skeleton == runtime.SKELETON_HMC
    tr = trace_callback(small, ex)
    assert c.generated == emit.value_grad_source(tr.graph, tr.value, tr.grad(), "f64", 0)           # the straight-line text, as before
    big = cases.big_logistic()
    ex4 = torch.full((4,), 0.1, dtype=f64)
    c = jit.compile_hmc(big, ex4, f64, 0)                                  # refused for its size before: "value + gradient are N scalar operations"
    assert isinstance(c, jit.CompiledRolled) and c.rolled.rows == [1500] and c.skeleton == runtime.SKELETON_ROLLED
    assert c.traced._grad is None                                          # the unrolled graph was never differentiated
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_ROLL", "0")
    with pytest.raises(Unsupported, match=r"value \+ gradient are \d+ scalar operations \(limit 6000\)"):
        jit.compile_hmc(cases.big_logistic(N=400), ex4, f64, 0)
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_ROLL", "force")
    assert isinstance(jit.compile_hmc(cases.logistic(N=12, D=3, seed=4), ex, f64, 0), jit.CompiledRolled)
    c = jit.compile_hmc(lambda w: -(w ** 4).sum() - torch.exp(w[0]), ex, f64, 0)                    # nothing to roll: straight-line
    assert type(c) is jit.CompiledHMC


def test_refusals_carry_their_reason(monkeypatch):
    tr = trace_callback(cases.logistic(), torch.full((3,), 0.2, dtype=f64))
    with pytest.raises(Unsupported, match=r"group of 40 rows is \d+ scalar operations with its gradient \(limit 10\)"):
        roll.roll(tr.graph, tr.value, 10)
    trh = trace_callback(_heavy_rest(), torch.full((3,), 0.2, dtype=f64))
    with pytest.raises(Unsupported, match=r"what was not rolled are \d+ scalar operations with their gradient \(limit 40\)"):
        roll.roll(trh.graph, trh.value, 40)             # (the term of its 40 rows, 21 operations, passes)
    rng = np.random.default_rng(0)
    A, B = torch.tensor(rng.standard_normal((10, 40))), torch.tensor(rng.standard_normal((10, 40)))

    def wide(w):
        return -torch.exp(A @ w + B @ (w * w)).sum()
    trw = trace_callback(wide, torch.full((40,), 0.1, dtype=f64))
    with pytest.raises(Unsupported, match=r"40 nodes are shared between the rows \(limit 32 uniforms\)"):       # the squares w_j^2
        roll.roll(trw.graph, trw.value, runtime.MAX_HMC_NODES)
    trw = trace_callback(lambda w: -torch.exp((A @ w) * (B @ w)).sum(), torch.full((40,), 0.1, dtype=f64))
    with pytest.raises(Unsupported, match=r"80 constants that differ between rows \(limit 64 slots\)"):
        roll.roll(trw.graph, trw.value, runtime.MAX_HMC_NODES)
    with pytest.raises(Unsupported, match=r"nothing to roll"):
        roll.roll(*(lambda t: (t.graph, t.value))(trace_callback(lambda w: -(w ** 4).sum(), torch.ones(3, dtype=f64))), 6000)
    # a callable that compiles in its rolled form only, asked of the routes that have no rolled form
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_ROLL", "auto")
    ex4 = torch.full((4,), 0.1, dtype=f64)
    big = cases.big_logistic()
    with pytest.raises(Unsupported, match=r"rolled over its 1500 data rows .* not for leapfrog\(\) paths"):
        jit.compile_path(big, ex4, f64, 0)
    assert "leapfrog() paths" in jit.last_reason()
    assert isinstance(jit.compile_hmc(big, ex4, f64, 0), jit.CompiledRolled)            # ... and sample() still gets the rolled kernel
    with pytest.raises(Unsupported, match=r"subset 1: the value alone is \d+ scalar operations .* not for lists of callables"):
        jit.compile_split([cases.logistic(D=4), big], ex4, f64, 0)
    with pytest.raises(Unsupported, match=r"the value alone is \d+ scalar operations .* not for the derivative and RMHMC kernels"):
        jit.compile_derivs(big, ex4, f64)


def _heavy_rest():
    f = cases.logistic()

    def g(w):
        return f(w) - torch.exp(torch.sin(w[0] * w[1]) * torch.cos(w[2] * w[0])) - torch.tanh(w[1] * w[2]) ** 2 - torch.log1p(w[0] * w[0]) * torch.atan(w[1])
    return g


def inspect(blob, tmp_path):
    p = tmp_path / "cb.co"
    p.write_bytes(blob)
    sym = subprocess.run([READELF, "-s", str(p)], capture_output=True, text=True).stdout
    notes = subprocess.run([READELF, "--notes", str(p)], capture_output=True, text=True).stdout
    names = set(re.findall(r"\b(hta_cb_\w+?)(?:\.kd)?\b", sym))
    blocks = re.split(r"\n\s+- \.agpr_count", notes)
    mine = next(b for b in blocks if re.search(r"\.name:\s+hta_cb_rolled_kernel\b", b))
    regs = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)", mine)}
    return names, regs


def info_words(blob, tmp_path):
    """hta_cb_info's eight words, read from the code object's data section."""
    p = tmp_path / "cb.co"
    p.write_bytes(blob)
    sym = subprocess.run([READELF, "-s", str(p)], capture_output=True, text=True).stdout
    sec = subprocess.run([READELF, "-S", str(p)], capture_output=True, text=True).stdout
    m = re.search(r"^\s*\d+:\s+([0-9a-f]+)\s+32\s+OBJECT\s+\S+\s+\S+\s+(\d+)\s+hta_cb_info\s*$", sym, re.M)
    addr, shndx = int(m.group(1), 16), int(m.group(2))
    s = re.search(r"\[\s*%d\]\s+\S+\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+" % shndx, sec)
    off = int(s.group(2), 16) + addr - int(s.group(1), 16)
    return list(np.frombuffer(blob[off:off + 32], dtype=np.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case,D", [("logistic", 3), ("hierarchical", 4)])
def test_the_rolled_kernel_compiles_for_gfx950(case, D, dtype, tmp_path):
    _, R = rolled(getattr(cases, case)(), D)
    src = runtime.rolled_generated_source(R, dtype, 0)
    key, blob = runtime.compile_source(src, runtime.SKELETON_ROLLED)
    names, regs = inspect(blob, tmp_path)
    assert names == {"hta_cb_rolled_kernel", "hta_cb_predraw_kernel", "hta_cb_info"}, names
    item = 4 if dtype == torch.float32 else 8
    assert info_words(blob, tmp_path) == [0x48544131, D, item, 0, 6, sum(g.live for g in R.groups) + R.rest_live, R.U, len(R.groups)]
    assert regs["max_flat_workgroup_size"] == 64 * runtime.rolled_max_waves(D, item)
    assert regs["vgpr_spill_count"] == 0 and regs["private_segment_fixed_size"] == 0, regs          # (asked of case 1 in float32; holds for all four)
    assert runtime.compile_source(src, runtime.SKELETON_ROLLED)[0] == key                           # cached by content


def test_no_scratch_at_eight_dimensions_two_uniforms_ten_slots(tmp_path):
    """The resource target: D = 8, U = 2, S = 10 in float32 - no scratch, no spilled vector register, at the 16-wave launch bound."""
    rng = np.random.default_rng(3)
    X, Z, y = (torch.tensor(rng.standard_normal(s), dtype=f64) for s in ((32, 6), (32, 3), (32,)))

    def fn(th):             # a row's mean has 6 + 3 coefficients, its datum is the tenth slot; th[6] and th[7] make the two shared nodes
        r = y - X @ th[:6] - torch.tanh(th[7]) * (Z @ th[:3])
        return -0.5 * (torch.exp(-2.0 * th[6]) * r * r).sum() - 32.0 * th[6] - 0.5 * (th * th).sum()
    _, R = rolled(fn, 8)
    assert R.rows == [32] and R.U == 2 and R.groups[0].slots == 10, (R.rows, R.U, [g.slots for g in R.groups])
    against_autograd(fn, R, 8)
    _, blob = runtime.compile_source(runtime.rolled_generated_source(R, torch.float32, 0), runtime.SKELETON_ROLLED)
    _, regs = inspect(blob, tmp_path)
    assert regs["max_flat_workgroup_size"] == 1024 and regs["vgpr_spill_count"] == 0 and regs["private_segment_fixed_size"] == 0, regs


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_the_lds_form_of_the_table_reads_compiles(dtype, tmp_path, monkeypatch):
    """HAMILTORCH_AMD_JIT_ROLL_TABLE=lds: another text (HTA_CB_TABLE_LDS 1), another code object, the same exports, no scratch."""
    _, R = rolled(cases.two_structures(), 3)
    direct = runtime.rolled_generated_source(R, dtype, 0)
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_ROLL_TABLE", "lds")
    src = runtime.rolled_generated_source(R, dtype, 0)
    assert "#define HTA_CB_TABLE_LDS 1" in src and "#define HTA_CB_TABLE_LDS 0" in direct
    assert src.replace("HTA_CB_TABLE_LDS 1", "HTA_CB_TABLE_LDS 0") == direct
    key, blob = runtime.compile_source(src, runtime.SKELETON_ROLLED)
    assert key != runtime.compile_source(direct, runtime.SKELETON_ROLLED)[0]
    names, regs = inspect(blob, tmp_path)
    assert names == {"hta_cb_rolled_kernel", "hta_cb_predraw_kernel", "hta_cb_info"}, names
    assert regs["vgpr_spill_count"] == 0 and regs["private_segment_fixed_size"] == 0, regs


def test_unset_the_switch_keeps_the_previous_behaviour(monkeypatch):
    """Without rates measured against the torch-evaluated route the rolled route is opt-in: unset, a large likelihood is refused for its
    size as before."""
    monkeypatch.delenv("HAMILTORCH_AMD_JIT_ROLL", raising=False)
    assert runtime.ROLL_DEFAULT == "0" and runtime.roll_mode() == "0"
    with pytest.raises(Unsupported, match=r"value \+ gradient are \d+ scalar operations \(limit 6000\)"):
        jit.compile_hmc(cases.big_logistic(N=300, seed=12), torch.full((4,), 0.1, dtype=f64), f64, 0)


def test_the_switches_are_part_of_the_trace_cache_key(monkeypatch):
    """An entry made under one setting of HAMILTORCH_AMD_JIT_ROLL is not handed out under another: '0' set later in the process still
    reproduces the straight-line route, and a callable first seen by compile_path under 'force' still rolls for sample()."""
    fn, ex = cases.logistic(N=16, seed=8), torch.full((3,), 0.2, dtype=f64)
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_ROLL", "force")
    assert isinstance(jit.compile_path(fn, ex, f64, 0), jit.CompiledPath)               # straight-line: paths have no rolled form
    assert isinstance(jit.compile_hmc(fn, ex, f64, 0), jit.CompiledRolled)
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_ROLL", "0")
    assert type(jit.compile_hmc(fn, ex, f64, 0)) is jit.CompiledHMC
    monkeypatch.setenv("HAMILTORCH_AMD_JIT_ROLL", "force")
    assert isinstance(jit.compile_hmc(fn, ex, f64, 0), jit.CompiledRolled)
    c = jit.compile_hmc(lambda w: -(w ** 4).sum(), ex, f64, 0)
    assert type(c) is jit.CompiledHMC                                                   # nothing to roll under 'force': straight-line


def test_a_heavy_term_gets_registers_instead_of_waves():
    M = runtime.rolled_max_waves
    assert M(8, 4, 51) == 16 and M(8, 4, 200) == 8 and M(8, 4, 3000) == 4 and M(40, 4, 30) == 4
    assert M(8, 8, 51) == 8 and M(8, 8, 500) == 4
    assert runtime.rolled_waves(1024, 8, 0, 2000, 4, live=3000) == 4


def test_the_wave_rule():
    W = runtime.rolled_waves
    assert W(1024, 8, 0, 2000, 4) == 16                  # 16 blocks x 16 waves
    assert W(65536, 8, 0, 2000, 4) == 2                  # 1024 blocks: 2048 waves at most
    assert W(1 << 20, 8, 0, 2000, 4) == 1
    assert W(1024, 8, 0, 40, 4) == 4                     # at least 8 rows per wave
    assert W(1024, 64, 32, 2000, 8) == 1                 # 2 x 64 x 97 x 8 bytes are beyond 64 KB
    assert W(1024, 8, 0, 2000, 8) == 8                   # float64: the kernel is built for 8 waves
    for C, D, U, rows, item in ((1024, 8, 0, 2000, 4), (64, 64, 32, 100000, 8), (130, 3, 0, 40, 8)):
        w = W(C, D, U, rows, item)
        assert w in runtime.ROLLED_WAVES and (w * 64 * (1 + D + U) * item <= runtime.ROLLED_LDS or w == 1)


def test_the_code_cache_is_bounded():
    assert runtime.MAX_CODE == 64
    saved = dict(runtime._code)
    try:
        runtime._code.clear()
        runtime._code.update({"k%d" % i: b"x" for i in range(64)})
        _, R = rolled(cases.logistic(), 3)
        key, _ = runtime.compile_source(runtime.rolled_generated_source(R, torch.float32, 1), runtime.SKELETON_ROLLED)
        assert len(runtime._code) == 64 and key in runtime._code and "k0" not in runtime._code and "k1" in runtime._code
    finally:
        runtime._code.clear()
        runtime._code.update(saved)


def test_the_entry_point_refuses_bad_arguments_without_a_device():
    lib = _abi.load()
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.addressof(buf)

    def call(D_=3, U=0, groups=1, itemsize=8, mass=0, table=(ptr,), rows=(40,), **kw):
        a = _abi.HtaCbRolledArgs()
        a.cur = a.init = a.reject_count = ptr
        a.C, a.eps, a.L, a.n_traj, a.waves = 1, 0.1, 1, 1, 2
        for k, (t, r) in enumerate(zip(table, rows)):
            a.table[k], a.rows[k] = t, r
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.hta_jit_rolled_sample(None, ctypes.byref(a), D_, U, groups, itemsize, mass, ptr, 1 << 20, None)

    assert ctypes.sizeof(_abi.HtaCbRolledArgs) == ctypes.sizeof(_abi.HtaCbHmcArgs) + 4 * 8 + 4 * 4 + 8      # + tables, rows, waves (padded)
    assert _abi.HtaCbRolledArgs.table.offset == ctypes.sizeof(_abi.HtaCbHmcArgs)
    assert call() == -1 and "module is NULL" in _abi.last_error()            # good arguments get as far as the module
    for bad, why in ((dict(waves=3), "3 waves"), (dict(waves=0), "0 waves"), (dict(waves=32), "32 waves"),
                     (dict(table=(None,)), "table of group 0 is NULL"), (dict(groups=2, table=(ptr, None), rows=(40, 8)), "table of group 1 is NULL"),
                     (dict(rows=(0,)), "group 0 has 0 rows"), (dict(rows=(-4,)), "has -4 rows"),
                     (dict(D_=64, U=32, waves=2), "bytes of LDS (limit 65536)"), (dict(D_=64, U=0, itemsize=8, waves=4), "bytes of LDS"),
                     (dict(groups=5), "5 groups"), (dict(groups=0), "0 groups"), (dict(C=0), "bad arguments"), (dict(cur=None), "bad arguments"),
                     (dict(itemsize=2), "bad arguments"), (dict(mass=1), "mass operands are NULL")):
        assert call(**bad) == -1, bad
        assert why in _abi.last_error() and "module is NULL" not in _abi.last_error(), (bad, _abi.last_error())
    assert lib.hta_jit_rolled_sample(None, None, 3, 0, 1, 8, 0, ptr, 1 << 20, None) == -1


# ---- the oracle side of tests/test_gpu_jit_roll.py -------------------------------------------------------------------------------
@pytest.mark.parametrize("case,D,kw", [("logistic", 3, {}), ("logistic", 3, dict(N=3)), ("hierarchical", 4, {}), ("hierarchical", 4, dict(N=300)),
                                       ("two_structures", 3, {}), ("two_structures", 3, dict(n=7, n_gauss=19)), ("big_logistic", 4, {})])
def test_the_oracle_targets_against_autograd(case, D, kw):
    """The closed forms of jit_roll_cases.py, batched, against torch.autograd of the callable in float64 at a dozen points: the bound of
    `against_autograd`, 1e-10 relative to 1 + |ref|.  A float32 theta is evaluated in float32 and comes back as float32."""
    fn = getattr(cases, case)(**kw)
    tgt = cases.oracle_target(fn)
    pts = 0.5 * np.random.default_rng(7).standard_normal((12, D))
    mine = np.concatenate([tgt.logp(pts)[:, None], tgt.grad(pts)], 1)
    assert mine.shape == (12, 1 + D) and mine.dtype == np.float64
    for k in range(12):
        x = torch.tensor(pts[k], dtype=f64, requires_grad=True)
        v = fn(x)
        g, = torch.autograd.grad(v, x)
        ref = np.concatenate([[float(v.detach())], g.numpy()])
        assert np.all(np.abs(mine[k] - ref) <= 1e-10 * (1.0 + np.abs(ref))), (k, mine[k], ref)
        one = np.concatenate([[tgt.logp(pts[k])], tgt.grad(pts[k])])                    # a single point, [D]
        assert np.all(np.abs(one - ref) <= 1e-10 * (1.0 + np.abs(ref)))
    low = pts.astype(np.float32)
    assert tgt.logp(low).dtype == np.float32 and tgt.grad(low).dtype == np.float32
    assert np.all(np.abs(tgt.grad(low) - mine[:, 1:]) <= 1e-4 * (1.0 + np.abs(mine[:, 1:])))


def flipped_and_deviation(run):
    """The float32 oracle against the float64 oracle on the same start, mass matrix and draws: which chains took another accept
    decision somewhere, and the largest difference per chain."""
    (a, ia), (b, ib) = run.oracle(torch.float32), run.oracle(torch.float32, exact=True)
    flipped = (np.stack(ia["accept"]) != np.stack(ib["accept"])).any(0)
    return flipped, cases.deviation(a, b), ia


@pytest.mark.parametrize("name", [n for n in cases.F32_RUNS if n != "long"])
def test_the_float32_oracle_is_inside_the_band_and_the_cap(name):
    """Every float32 run of tests/test_gpu_jit_roll.py is judged at 2e-4 with 3 % of the chains exempt.  That judges the kernel only if
    float32 ARITHMETIC on that run - the oracle evaluated in float32 against the oracle in float64, same draws - is well inside both:
    no chain that kept its accept decisions beyond a third of the band, flipped chains within a third of the cap (1 chain in 100)."""
    run = cases.RUNS[name]
    flipped, err, info = flipped_and_deviation(run)
    print("%s: %d of %d chains flipped, largest deviation of the others %.3g, acceptance %.2f"
          % (name, flipped.sum(), flipped.size, err[~flipped].max(), info["acc_rate"].mean()))
    assert flipped.mean() <= cases.MAX_FLIPPED / 3
    assert err[~flipped].max() <= cases.TOL[torch.float32] / 3
    assert (err > cases.TOL[torch.float32]).mean() <= cases.MAX_FLIPPED / 3


def test_the_float32_bound_of_the_long_sums():
    """1500 rows in float32: the bound of test_long_sums is 4 x the deviation of the float32 oracle from the float64 oracle MEASURED
    here (LONG_F32_MEASURED, recorded next to that test) - this test keeps the record honest: what it measures is not above it, and
    the run moves (the oracle accepts between 0.5 and 1.0 of its proposals)."""
    import test_gpu_jit_roll as G
    run = cases.RUNS["long"]
    flipped, err, info = flipped_and_deviation(run)
    print("long: %d of %d chains flipped, largest deviation of the others %.4g, acceptance %.3f"
          % (flipped.sum(), flipped.size, err[~flipped].max(), info["acc_rate"].mean()))
    assert flipped.mean() <= cases.MAX_FLIPPED / 3
    assert 0.5 * G.LONG_F32_MEASURED <= err[~flipped].max() <= G.LONG_F32_MEASURED
    assert G.LONG_F32_BOUND == 4 * G.LONG_F32_MEASURED
    for dtype in (torch.float32, f64):
        acc = run.oracle(dtype)[1]["acc_rate"].mean()
        assert 0.5 <= acc <= 1.0, acc
