"""CPU: the propagator coefficients of the quad route (hamiltorch_amd/csrc/quad_prop.hpp: quad_prop_coeffs) from a stand-alone host
program built around the header, against numpy's float64 recurrence rounded to float32 (tests/quad_prop_ref.py:coeffs) - bit for bit.

Cases: L = 0, 1, 2, 5, 7, 25, 100, 1000 times eps sqrt(lam) = f x 2 (2: the leapfrog's stability limit) for f = 0.01 ... 0.99, at the
limit (1), beyond it (1.01, 1.5, 4), lam = 0 with a live step size, and the dummy lane (eps = lam = 0), at three eigenvalues.

Determinant.  The exact map is symplectic: ad - bc = 1.  The float64 recurrence keeps that to float64 rounding, and each float32
coefficient is off by at most half an ulp of itself (2^-24 relative), so |ad - bc - 1| <= 2^-23 (|ad| + |bc|) + O(2^-47).  Asserted:
4 ulp of 1 (4 x 2^-23) times max(1, |ad| + |bc|); the factor is 1 wherever the step is stable and away from the limit (a = d = cos,
bc = -sin^2), and only the growing maps at and beyond the limit scale the bound.  Maps with a non-finite coefficient (float32
overflow, L = 1000 beyond the limit) are held to the bits only."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import quad_prop_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hamiltorch_amd", "csrc")
LS = (0, 1, 2, 5, 7, 25, 100, 1000)
FRACTIONS = (0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99, 1.0, 1.01, 1.5, 4.0)
LAMS = (0.5, 1.37, 2.0)

MAIN = r"""
#include <cstdio>
#include <cstdint>
#include <cstring>
#include "quad_prop.hpp"
static float f_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t u_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
int main() {
  unsigned e, n, h; int L;
  while (scanf("%x %x %x %d", &e, &n, &h, &L) == 4) {
    const hta::QuadProp p = hta::quad_prop_coeffs(f_of(e), f_of(n), f_of(h), L);
    printf("%08x %08x %08x %08x\n", u_of(p.a), u_of(p.b), u_of(p.c), u_of(p.d));
  }
  return 0;
}
"""


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _cases():
    out = []
    for L in LS:
        for lam in LAMS:
            for f in FRACTIONS:
                out.append(R.lane_constants(np.float32(2.0 * f / np.sqrt(lam)), lam) + (L,))
        out.append(R.lane_constants(0.3, 0.0) + (L,))                  # lam = 0: a free coordinate
        out.append((np.float32(0), np.float32(-0.0), np.float32(0), L))      # the dummy lane: eps = lam = 0, nel = -(0 * 0)
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not (shutil.which(cxx) or os.path.exists(cxx)):
        pytest.skip("needs a host C++ compiler")
    d = tmp_path_factory.mktemp("quad_prop")
    (d / "main.cpp").write_text(MAIN)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC, "-o", str(d / "coeffs"), str(d / "main.cpp")],
                   check=True, capture_output=True)
    return str(d / "coeffs")


def test_coefficients_equal_the_float64_recurrence_rounded_to_float32(program):
    cases = _cases()
    text = "".join("%08x %08x %08x %d\n" % (_bits(e), _bits(n), _bits(h), L) for e, n, h, L in cases)
    out = subprocess.run([program], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
    assert len([ln for ln in out if ln]) == len(cases)
    worst = 0.0
    for (e, n, h, L), ln in zip(cases, out):
        got = tuple(int(w, 16) for w in ln.split())
        want = tuple(_bits(x) for x in R.coeffs(e, n, h, L))
        assert got == want, (float(e), float(n), float(h), L, ln, want)
        a, b, c, d = (float(x) for x in R.coeffs(e, n, h, L))
        if np.isfinite([a, b, c, d]).all():
            det = abs(a * d - b * c - 1.0)
            bound = 4.0 * 2.0 ** -23 * max(1.0, abs(a * d) + abs(b * c))
            if abs(a * d) + abs(b * c) <= 1.0 + 1e-6:
                worst = max(worst, det)
            assert det <= bound, (float(e), float(n), float(h), L, det, bound)
    print("largest |ad - bc - 1| over the maps with |ad| + |bc| <= 1: %.3g (4 ulp: %.3g)" % (worst, 4.0 * 2.0 ** -23))


def test_the_trivial_maps():
    """L = 0: the two half kicks cancel exactly (a = d = 1, b = 0, c = -hl + hl = 0); the dummy lane at any L: the identity."""
    e, n, h = R.lane_constants(0.3, 1.37)
    assert R.coeffs(e, n, h, 0) == (1.0, 0.0, 0.0, 1.0)
    for L in LS:
        assert R.coeffs(0.0, -0.0, 0.0, L) == (1.0, 0.0, 0.0, 1.0)
