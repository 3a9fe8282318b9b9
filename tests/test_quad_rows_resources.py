"""CPU: the code objects of the fused quad launch with row waves (csrc/hmc_gauss_quad_dev.hpp: hmc_gauss_quad_fused_kernel<D, LB, NI>,
tuning key "quad_rows") - no scratch, the LDS is exactly the hand-over ring, the registers do not exceed those of the launch
without row waves, and the integrating wave's hot loop keeps inside its instruction budget (read from the built library)."""
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
            if not name or "hmc_gauss_quad_fused_kernel" not in name.group(1):
                continue
            g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))      # noqa: E731
            out[name.group(1)] = dict(vgpr=g("vgpr_count"), sgpr=g("sgpr_count"), scratch=g("private_segment_fixed_size"),
                                      lds=g("group_segment_fixed_size"), spill=g("vgpr_spill_count"), threads=g("max_flat_workgroup_size"))
    return out


def _split(kernels):
    """{(D, LB): (instance without row waves, instance with row waves, NI)}"""
    out = {}
    for k, v in kernels.items():
        m = re.search(r"quad_fused_kernelILi(\d)ELi(\d+)ELi(\d)E", k)
        assert m, k
        D, LB, NI = int(m.group(1)), int(m.group(2)), int(m.group(3))
        e = out.setdefault((D, LB), [None, None, 0])
        if NI == 0:
            e[0] = v
        else:
            e[1], e[2] = v, NI
    return out


def test_row_wave_instances_have_no_scratch_and_exactly_the_ring_in_lds(kernels):
    pairs = _split(kernels)
    assert len(pairs) == 16                                   # D = 1 ... 4 x L = 25, 10, 5, any
    for (D, LB), (plain, rows, NI) in pairs.items():
        assert plain is not None and rows is not None, (D, LB)
        assert rows["scratch"] == 0 and rows["spill"] == 0, (D, LB, rows)
        assert plain["scratch"] == 0 and plain["lds"] == 0, (D, LB, plain)
        nu = 32 if LB == 25 else 16                           # trajectories per pass of the unrolled loop (quad_nu with four record slots)
        assert rows["lds"] == NI * 2 * nu * 64 * 4, (D, LB, rows)          # per integrating wave: two buffers of a pass x 64 lanes x 4 bytes
        assert rows["threads"] == 128 * NI, (D, LB, rows)
        # one kernel, two roles: its register count is that of the larger role, the integrating wave - which lost the row's
        # coefficients, offsets and element
        assert rows["vgpr"] <= plain["vgpr"], (D, LB, rows, plain)


def test_integrating_wave_keeps_inside_its_instruction_budget():
    """The time of a trajectory at BASELINE config 2 is the integrating wave's instruction count (one wave per SIMD: an issue slot
    each).  The hot loop of <3, 25> - 32 trajectories, 54 chain / energy FMAs each - held 73.25 instructions per
    trajectory with the rows on the integrating wave; without them at most 68, no memory instruction but the record load and the
    message's LDS write, and one barrier per pass."""
    obj = os.path.join(ROOT, "hamiltorch_amd", "csrc", "build", "hmc_gaussian.o")
    if not (os.path.exists(obj) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("needs the object file of hmc_gaussian.hip")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_of
    _, lines = isa_of.kernel_lines(obj, r"hmc_gauss_quad_fused_kernelILi3ELi25ELi[1-9]E", whole=True)
    hot = []
    for s_, e_ in isa_of.loops(lines):
        ops = [isa_of.classify(i) for _, i in lines[s_:e_ + 1]]
        if ops.count("fma") == 32 * 54:
            hot.append((e_ - s_ + 1, ops))
    assert hot
    n, ops = min(hot)
    assert n <= 32 * 68, n / 32.0
    assert ops.count("mem") == 32 and ops.count("lds") == 32 and ops.count("barrier") == 1, (ops.count("mem"), ops.count("lds"), ops.count("barrier"))
