"""CPU: the code objects of the quad route's propagator twins (csrc/hmc_gauss_quad_dev.hpp: quad_body PROP; tuning key "quad_prop"),
read from the built library and object in the manner of tests/test_quad_lead_resources.py.

The default launch at D = 3 is hmc_gauss_quad_lead_prop_kernel<3, 4> (512 threads, four chains per block).  Held here:
  - no scratch, no spill, 512 threads, and LDS of exactly the two rings: messages and records, two passes of 32 positions x 64 lanes x
    4 bytes each = 32 KB;
  - the integrating wave's pass of 32 trajectories: at most 24 instructions per trajectory, no global memory instruction, one barrier,
    eight 16-byte LDS reads and eight 16-byte LDS writes;
  - the trajectory itself is FOUR instructions in that pass: a trajectory's plain (non-DPP) arithmetic is the map's two multiplies and
    two FMAs (y = fma(b, z, a yc), r = fma(d, z, c yc)) plus what the energies take whatever the integrator - eo = fma(z, z, potc),
    pot1 = lam y y (two multiplies), en = fma(r, r, pot1) - so the pass holds exactly 32 x 4 FMAs and 32 x 4 multiplies, against
    32 x 54 FMAs of the step-by-step instance at L = 25;
  - every twin exists, for every D its form supports, with no scratch and no spill."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "hamiltorch_amd", "libhamiltorch_amd.so")
OBJ = os.path.join(ROOT, "hamiltorch_amd", "csrc", "build", "hmc_gaussian.o")
DEFAULT = r"hmc_gauss_quad_lead_prop_kernelILi3ELi4EE"
BUDGET = 24          # instructions per trajectory on the integrating wave


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: resources} of every ..._prop_kernel"""
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("needs the built library and the ROCm llvm tools")
    d = tmp_path_factory.mktemp("co")
    shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
    out = {}
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], cwd=d, check=True, capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name or not re.search(r"hmc_gauss_quad_(\w+_)?prop_kernel", name.group(1)):
                continue
            g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))      # noqa: E731
            out[name.group(1)] = dict(vgpr=g("vgpr_count"), scratch=g("private_segment_fixed_size"), lds=g("group_segment_fixed_size"),
                                      spill=g("vgpr_spill_count"), threads=g("max_flat_workgroup_size"))
    return out


def _some(kernels, pattern):
    got = {k: v for k, v in kernels.items() if re.search(pattern, k)}
    assert got, pattern
    return got


def test_every_twin_exists_without_scratch(kernels):
    for v in kernels.values():
        assert v["scratch"] == 0 and v["spill"] == 0, v
    for D in (1, 2, 3, 4):
        _some(kernels, r"hmc_gauss_quad_prop_kernelILi%dELb1ELi0EE" % D)                     # the per-trajectory outputs' instance
        for var in (0, 3, 7):
            _some(kernels, r"hmc_gauss_quad_prop_kernelILi%dELb0ELi%dEE" % (D, var))
        for ni in (0, 2):
            _some(kernels, r"hmc_gauss_quad_fused_prop_kernelILi%dELi%dEE" % (D, ni))
    for D in (1, 2, 3):
        for form, threads in (("local", 256), ("wide", 256)):
            for v in _some(kernels, r"hmc_gauss_quad_%s_prop_kernelILi%dEE" % (form, D)).values():
                assert v["threads"] == threads and v["lds"] == 32 * 1024, (form, D, v)
        for cpb in (4, 8, 16):
            for v in _some(kernels, r"hmc_gauss_quad_lead_prop_kernelILi%dELi%dEE" % (D, cpb)).values():
                assert v["threads"] == 512 and v["lds"] == 32 * 1024, (D, cpb, v)


def test_the_default_twin_has_no_scratch_and_lds_of_exactly_the_two_rings(kernels):
    (v,) = _some(kernels, DEFAULT).values()
    print(v)
    assert v["scratch"] == 0 and v["spill"] == 0 and v["threads"] == 512, v
    assert v["lds"] == 2 * (2 * 32 * 64 * 4), v


def test_the_integrating_waves_pass_holds_four_trajectory_instructions_inside_the_budget():
    if not (os.path.exists(OBJ) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("needs the object file of hmc_gaussian.hip")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_of
    _, lines = isa_of.kernel_lines(OBJ, DEFAULT, whole=True)
    hot = []
    for s_, e_ in isa_of.loops(lines):
        ins = [i for _, i in lines[s_:e_ + 1]]
        ops = [isa_of.classify(i) for i in ins]
        # the integrating wave's pass: the innermost loop with the 32 second-stage butterflies' compares
        if ops.count("barrier") == 1 and sum(i.startswith("v_cmp_ge_f32") for i in ins) == 32:
            hot.append((e_ - s_ + 1, ops, ins))
    assert hot
    n, ops, ins = min(hot)
    print("pass of 32 trajectories: %d instructions (%.2f per trajectory), budget %d" % (n, n / 32.0, BUDGET))
    assert n <= 32 * BUDGET, n
    assert ops.count("mem") == 0 and ops.count("barrier") == 1, (ops.count("mem"), ops.count("barrier"))
    assert ops.count("fma") == 32 * 4, ops.count("fma")
    mul = [i for i, o in zip(ins, ops) if o == "valu" and i.startswith("v_mul_f32")]
    assert len(mul) == 32 * 4, len(mul)
    plain = [i.split()[0] for i, o in zip(ins, ops) if o in ("fma", "valu")]
    arith = [p for p in plain if "_f32" in p and not p.startswith(("v_cndmask", "v_cmp", "v_mov"))]      # (float arithmetic; the pass also flips its two LDS buffers)
    # fma + mul + the 32 subtractions eo - en: no other arithmetic in the pass
    assert len(arith) == 32 * 9 and sum(p.startswith("v_sub_f32") for p in arith) == 32, sorted(set(arith))
    lds = [i.split()[0] for i, o in zip(ins, ops) if o == "lds"]
    assert len(lds) == 16 and lds.count("ds_write_b128") == 8 and lds.count("ds_read_b128") == 8, lds
