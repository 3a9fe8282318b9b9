"""CPU: the code objects of the wide quad launch with the keys "quad_lead" and "quad_rows_wt" (csrc/hmc_gauss_quad_dev.hpp:
hmc_gauss_quad_lead_kernel<D, LB>, the 512-thread launch, and hmc_gauss_quad_wide_kernel<D, LB>, its 256-thread parity partner) - no
scratch, 32 KB of LDS at <3, 25>, the registers of the wide instance before the keys existed, and the integrating wave's pass of 32
trajectories at that instance's instruction count: the keys add lanes that draw and change a store of the row wave, the
integrating wave's code is not theirs to touch (read from the built library and object, in the manner of
tests/test_quad_wide_resources.py)."""
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

# hmc_gauss_quad_wide_kernel<3, 25> of the commit before the keys (profiles/r11a_quad_wide.txt (3); its VGPR count read from that
# commit's library with llvm-readelf --notes)
PARENT_PASS_INSTRUCTIONS = 2132
PARENT_VGPRS = 49


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{(kind, D, LB): resources} of the wide and the lead instances"""
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
            m = name and re.search(r"hmc_gauss_quad_(wide|lead)_kernelILi(\d)ELi(\d+)EE", name.group(1))
            if not m:
                continue
            g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))      # noqa: E731
            out[(m.group(1), int(m.group(2)), int(m.group(3)))] = dict(
                vgpr=g("vgpr_count"), scratch=g("private_segment_fixed_size"), lds=g("group_segment_fixed_size"),
                spill=g("vgpr_spill_count"), threads=g("max_flat_workgroup_size"))
    return out


def test_lead_instances_have_no_scratch_eight_waves_and_the_wide_instances_lds(kernels):
    lead = {k[1:]: v for k, v in kernels.items() if k[0] == "lead"}
    assert set(lead) == {(D, LB) for D in (1, 2, 3) for LB in (25, 10, 5, 0)}
    for (D, LB), v in lead.items():
        assert v["scratch"] == 0 and v["spill"] == 0, (D, LB, v)
        assert v["threads"] == 512, (D, LB, v)
        assert v["lds"] == kernels[("wide", D, LB)]["lds"], (D, LB, v)
    for kind in ("wide", "lead"):
        v = kernels[(kind, 3, 25)]
        print(kind, v)
        assert v["lds"] == 32 * 1024, (kind, v)
        assert v["scratch"] == 0 and v["spill"] == 0, (kind, v)
        assert v["vgpr"] <= PARENT_VGPRS, (kind, v)


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


@pytest.mark.parametrize("kind", ["wide", "lead"])
def test_the_integrating_waves_pass_is_at_the_parents_instruction_count(kind):
    """The pass of 32 trajectories of <3, 25>: the parent's instruction count, no global memory instruction, one barrier, eight
    16-byte LDS writes and eight 16-byte LDS reads."""
    if not (os.path.exists(OBJ) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("needs the object file of hmc_gaussian.hip")
    n, ops, ins = _hot_loop(r"hmc_gauss_quad_%s_kernelILi3ELi25EE" % kind)
    print("%s: pass of 32 trajectories: %d instructions (%.2f per trajectory), parent %d" % (kind, n, n / 32.0, PARENT_PASS_INSTRUCTIONS))
    assert n <= PARENT_PASS_INSTRUCTIONS, n
    assert ops.count("mem") == 0 and ops.count("barrier") == 1, (ops.count("mem"), ops.count("barrier"))
    lds = [i.split()[0] for i, o in zip(ins, ops) if o == "lds"]
    assert len(lds) == 16 and lds.count("ds_write_b128") == 8 and lds.count("ds_read_b128") == 8, lds


def test_the_row_wave_has_a_write_through_store_and_a_plain_one():
    """quad_rows_body WT: the row wave of <3, 25> holds the sample row's store in both forms - global_store_dword with the sc1 bit
    (agent scope, write-through) for "quad_rows_wt" = 1 and the plain one for 0 - and no store carries nt."""
    if not (os.path.exists(OBJ) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("needs the object file of hmc_gaussian.hip")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_of
    for kind in ("wide", "lead", "local"):
        _, lines = isa_of.kernel_lines(OBJ, r"hmc_gauss_quad_%s_kernelILi3ELi25EE" % kind, whole=True)
        stores = [i for _, i in lines if i.startswith("global_store_dword ")]
        wt = [i for i in stores if re.search(r"\bsc1\b", i)]
        assert wt and len(wt) < len(stores), (kind, stores)
        assert not [i for i in stores if re.search(r"\bnt\b", i)], (kind, stores)
        assert not [i for i in wt if re.search(r"\bsc0\b", i)], (kind, wt)      # (sc0 sc1 would be system scope)
