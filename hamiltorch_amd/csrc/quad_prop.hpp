// Gaussian HMC, quad route: a trajectory's leapfrog steps as ONE linear map (included by hmc_gauss_quad_dev.hpp; plain C++, so a
// host program can include it alone: tests/test_quad_prop_coeffs.py does).
//
// On the quad route a lane integrates one eigen-coordinate, and eps, nel = -(eps lam) and hl = eps lam / 2 are constants of the
// launch.  The half kick, the L steps  y += eps r ; r += nel y  and the closing half kick take (yc, z) to (y, r) linearly:
//     y = a yc + b z        r = c yc + d z
// quad_prop_coeffs runs exactly that straight-line arithmetic in float64 on the basis inputs (1, 0) and (0, 1), with the float32
// constants the kernel holds promoted to double, and rounds the four results to float32.  "The same code on basis vectors" covers
// every mass kind and whitening (they only change lam), the dummy lane (eps = lam = 0: a = d = 1, b = c = 0) and every L >= 0 with
// no special case.  Multiplies and adds are kept apart (no contraction), so host, device and a numpy restatement give the same bits.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HTA_QUAD_PROP_HD __host__ __device__
#else
#define HTA_QUAD_PROP_HD
#endif

namespace hta {

struct QuadProp { float a, b, c, d; };

HTA_QUAD_PROP_HD inline QuadProp quad_prop_coeffs(float eps32, float nel32, float hl32, int L) {
#pragma clang fp contract(off)
  const double eps = (double)eps32, nel = (double)nel32, hl = (double)hl32;
  double y0 = 1.0, r0 = 0.0 - hl * 1.0;       // yc = 1, z = 0:  r = z - hl yc
  double y1 = 0.0, r1 = 1.0 - hl * 0.0;       // yc = 0, z = 1
  for (int l = 0; l < L; ++l) {
    y0 = y0 + eps * r0; r0 = r0 + nel * y0;
    y1 = y1 + eps * r1; r1 = r1 + nel * y1;
  }
  r0 = r0 + hl * y0;
  r1 = r1 + hl * y1;
  return QuadProp{(float)y0, (float)y1, (float)r0, (float)r1};
}

}  // namespace hta
