"""CPU: the code objects of the local quad launch (csrc/hmc_gauss_quad_dev.hpp: hmc_gauss_quad_local_kernel<D, LB>, tuning key "quad_local")
- no scratch, four waves, the LDS is exactly the message ring plus the record ring, and the integrating wave's hot loop reads its
records from LDS inside the instruction budget of the cross-block launch (read from the built library)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "hamiltorch_amd", "libhamiltorch_amd.so")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
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
            if not name or "hmc_gauss_quad_local_kernel" not in name.group(1):
                continue
            g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))      # noqa: E731
            out[name.group(1)] = dict(vgpr=g("vgpr_count"), scratch=g("private_segment_fixed_size"), lds=g("group_segment_fixed_size"),
                                      spill=g("vgpr_spill_count"), threads=g("max_flat_workgroup_size"))
    return out


def test_local_instances_have_no_scratch_four_waves_and_exactly_the_two_rings_in_lds(kernels):
    seen = set()
    for k, v in kernels.items():
        m = re.search(r"quad_local_kernelILi(\d)ELi(\d+)EE", k)
        assert m, k
        D, LB = int(m.group(1)), int(m.group(2))
        seen.add((D, LB))
        assert v["scratch"] == 0 and v["spill"] == 0, (D, LB, v)       # (what tests/test_quad_rows_resources.py holds the cross-block instances to)
        assert v["threads"] == 256, (D, LB, v)
        nu = 32 if LB == 25 else 16                           # trajectories per pass of the unrolled loop
        msgs = 2 * nu * 64 * 4                                # two buffers of a pass x 64 lanes x 4 bytes
        recs = 2 * nu * 16 * 16                               # two buffers of a pass x 16 chains x one 16-byte record
        assert v["lds"] == msgs + recs, (D, LB, v)
    assert seen == {(D, LB) for D in (1, 2, 3) for LB in (25, 10, 5, 0)}


def test_local_integrating_wave_reads_lds_only_inside_the_parents_budget():
    """The hot loop of <3, 25> - 32 trajectories, 54 chain / energy FMAs each: at most the 68 instructions per trajectory the
    cross-block launch is held to (tests/test_quad_rows_resources.py), no global memory instruction at all, 64 LDS instructions
    (a message write and a record read per trajectory) and one barrier per pass."""
    obj = os.path.join(ROOT, "hamiltorch_amd", "csrc", "build", "hmc_gaussian.o")
    if not (os.path.exists(obj) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("needs the object file of hmc_gaussian.hip")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_of
    _, lines = isa_of.kernel_lines(obj, r"hmc_gauss_quad_local_kernelILi3ELi25EE", whole=True)
    hot = []
    for s_, e_ in isa_of.loops(lines):
        ins = [i for _, i in lines[s_:e_ + 1]]
        ops = [isa_of.classify(i) for i in ins]
        if ops.count("fma") == 32 * 54:
            hot.append((e_ - s_ + 1, ops, ins))
    assert hot
    n, ops, ins = min(hot)
    assert n <= 32 * 68, n / 32.0
    assert ops.count("mem") == 0 and ops.count("lds") == 64 and ops.count("barrier") == 1, (ops.count("mem"), ops.count("lds"), ops.count("barrier"))
    lds = [i.split()[0] for i, o in zip(ins, ops) if o == "lds"]
    assert lds.count("ds_write_b32") == 32 and lds.count("ds_read_b32") == 32, lds
