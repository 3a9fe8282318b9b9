"""CPU: the code objects of the wide quad launch (csrc/hmc_gauss_quad_dev.hpp: hmc_gauss_quad_wide_kernel<D, LB>, tuning key "quad_wide") -
no scratch, four waves, the LDS of the local instance, and the integrating wave's hot loop of <3, 25> hands over with 16 LDS
instructions of 16 bytes per pass, inside the instruction count of the local kernel's hot loop in the same object and inside its
registers plus the eight record registers (read from the built library and object)."""
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


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{(kind, D, LB): resources} of the local and the wide instances"""
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
            m = name and re.search(r"hmc_gauss_quad_(local|wide)_kernelILi(\d)ELi(\d+)EE", name.group(1))
            if not m:
                continue
            g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))      # noqa: E731
            out[(m.group(1), int(m.group(2)), int(m.group(3)))] = dict(
                vgpr=g("vgpr_count"), scratch=g("private_segment_fixed_size"), lds=g("group_segment_fixed_size"),
                spill=g("vgpr_spill_count"), threads=g("max_flat_workgroup_size"))
    return out


def test_wide_instances_have_no_scratch_four_waves_and_the_local_instances_lds(kernels):
    wide = {k[1:]: v for k, v in kernels.items() if k[0] == "wide"}
    assert set(wide) == {(D, LB) for D in (1, 2, 3) for LB in (25, 10, 5, 0)}
    for (D, LB), v in wide.items():
        assert v["scratch"] == 0 and v["spill"] == 0, (D, LB, v)
        assert v["threads"] == 256, (D, LB, v)
        assert v["lds"] == kernels[("local", D, LB)]["lds"], (D, LB, v)


def _hot_loop(kernel):
    """(instruction count, classes, instructions) of the kernel's loop with 32 x 54 FMAs: the integrating wave's pass of 32 trajectories"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_of
    _, lines = isa_of.kernel_lines(OBJ, kernel, whole=True)
    hot = []
    for s_, e_ in isa_of.loops(lines):
        ins = [i for _, i in lines[s_:e_ + 1]]
        ops = [isa_of.classify(i) for i in ins]
        if ops.count("fma") == 32 * 54:
            hot.append((e_ - s_ + 1, ops, ins))
    assert hot, kernel
    return min(hot)


def test_wide_integrating_wave_hands_over_in_sixteen_byte_lds_instructions(kernels):
    """The hot loop of <3, 25>: no global memory instruction, one barrier, exactly 16 LDS instructions (a 16-byte message write and a
    16-byte record read per block of four trajectories), no more instructions than the local kernel's hot loop in the same object,
    and no more VGPRs than the local instance plus the eight record registers."""
    if not (os.path.exists(OBJ) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("needs the object file of hmc_gaussian.hip")
    n, ops, ins = _hot_loop(r"hmc_gauss_quad_wide_kernelILi3ELi25EE")
    n_local, _, _ = _hot_loop(r"hmc_gauss_quad_local_kernelILi3ELi25EE")
    print("hot loop: wide %d instructions (%.2f per trajectory), local %d (%.2f)" % (n, n / 32.0, n_local, n_local / 32.0))
    assert ops.count("mem") == 0 and ops.count("barrier") == 1, (ops.count("mem"), ops.count("barrier"))
    lds = [i.split()[0] for i, o in zip(ins, ops) if o == "lds"]
    assert len(lds) == 16 and lds.count("ds_write_b128") == 8 and lds.count("ds_read_b128") == 8, lds
    assert n <= n_local, (n, n_local)
    assert kernels[("wide", 3, 25)]["vgpr"] <= kernels[("local", 3, 25)]["vgpr"] + 8, (kernels[("wide", 3, 25)], kernels[("local", 3, 25)])


def test_wide_second_butterfly_stages_have_their_two_wait_states():
    """A DPP read of a register the instruction before wrote needs two wait states, and the compiler does not look into the asm
    blocks of the accept tail: in the first trajectory of a block the wait states of the second stage are LDS accesses (or an
    s_nop) the compiler places between two asm blocks.  In the built code of wide instances of every D and pass length, every second stage
    (quad_perm:[2,3,0,1]) of the integrating wave's butterfly has at least two wait states since its first stage ([1,0,3,2])."""
    if not (os.path.exists(OBJ) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("needs the object file of hmc_gaussian.hip")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_of
    for D, LB in ((3, 25), (3, 0), (2, 5), (1, 10)):      # (the flagship, the any-L instance, every D, every pass length; a disassembly each)
        if True:
            _, lines = isa_of.kernel_lines(OBJ, r"hmc_gauss_quad_wide_kernelILi%dELi%dEE" % (D, LB), whole=True)
            ins = [i for _, i in lines]
            seen = 0
            for n, i in enumerate(ins):
                if not (i.startswith("v_add_f32_dpp") and "quad_perm:[2,3,0,1]" in i):
                    continue
                reg = i.split()[1].rstrip(",")
                states, m = 0, n - 1
                while m >= 0 and not (ins[m].startswith("v_add_f32_dpp") and "quad_perm:[1,0,3,2]" in ins[m] and ins[m].split()[1].rstrip(",") == reg):
                    states += int(ins[m].split()[1], 0) + 1 if ins[m].startswith("s_nop") else 1
                    m -= 1
                    if states > 8:
                        break
                assert m >= 0 and states >= 2, (D, LB, n, ins[max(n - 4, 0):n + 1])
                seen += 1
            assert seen >= 16, (D, LB, seen)          # (at least the pass of 16 or 32 trajectories)
