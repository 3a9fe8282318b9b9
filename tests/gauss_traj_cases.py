"""Cases for the trajectory-mode tests of the plain-HMC kernels for Gaussian targets - hmc_gauss_small_kernel<T,D,MASS,WS,DIAG>,
hmc_gauss_eig_kernel<T,D,DIAG>, hmc_gauss_quad_kernel<D,DIAG,LB[,VAR]>, the one-launch quad route (hmc_gauss_quad_fused_kernel<D,LB>),
hmc_gauss_wave_kernel<T,R,MASS> and hmc_gauss_wave_eig_kernel<T,R> (hamiltorch_amd/csrc/hmc_gaussian.hip) - and the driver that runs
oracle/hmc_oracle.py on them.  Plain numpy, no GPU, nothing of the library on the reference side.  Shared by
tests/test_gauss_traj_cases_cpu.py (which checks on the oracle alone that every case can tell a wrong kernel from a right one, and the
launcher's rules restated here against the table) and tests/test_gpu_gauss_traj.py (the kernels through hamiltorch_amd/_abi.py).
Same shape as tests/rmhmc_traj_cases.py.

TARGET.  P = Q diag(linspace(.5, 2, D)) Q^T rounded to float32 (Q from numpy's QR of a seeded normal matrix), mean linspace(-1, 1, D),
log_norm = -1 - D / 4, starts mu + 0.3 z with z the Philox INIT normals of (seed, chain id), chain offset 5, 8 trajectories, burn 2
unless the case says otherwise.  Mass operands as tests/test_gpu_hmc.py:masses builds them (inv_mass: a uniform(0.5, 2) diagonal, or
Q' diag(linspace(.5, 1.5, D)) Q'^T), rounded to float32.  The REFERENCE is oracle/hmc_oracle.py:sample_hmc in float64 started from those
float32 numbers cast up, for the float32 and the float64 kernels alike.

LAUNCHER.  gaussian_dispatch, launch_small, quad_route, quad_fused_route, wave_eig_route and hta_hmc_gaussian_workspace_bytes of
hamiltorch_amd/csrc/hmc_gaussian.hip are restated below (expected_route, workspace_bytes); the GPU tests hold them to the launcher through
_abi.last_route().  A ROUTE is a dict of tuning keys plus the workspace (no / yes / prepared) plus whether the per-trajectory outputs
(H_old, H_new, accept) are asked for plus the state dtype.  What the launcher does NOT have: a way to reach hmc_gauss_quad_kernel<D,false,LB>
without VAR other than quad_variant = 0 (a parity partner of tests/test_gpu_hmc.py, not run here), and no launch of the one-launch quad
route with fewer than 8 trajectories - a run of 8 cut in two leaves it (see TWO LAUNCHES).

BOUNDS (the project's own; none is fitted to what a GPU returned).  Sample rows, `cur` and the reset row: float32 2e-4 max(1,
|want|.max()) on the register-resident kernels (tests/test_gpu_hmc.py:test_sample_fused_vs_oracle), 3e-4 on the wave kernels
(test_wave_eigenbasis_route_vs_direct_and_oracle), 5e-4 from D = 257 (test_edge_sizes_against_oracle); float64 1e-10 and 1e-9.  At most
5 % of the compared chains outside in float32 (none of 9 .. 19, 1 of 31, 3 of 63 .. 65), none in float64.  H_old / H_new of trajectory 0
on every chain: 10 tol (|H| + 1 + D) with tol 2e-5 / 1e-11 (test_leapfrog_batch_vs_oracle's tolerance of `hamiltonian`), in float32
tightened per case to 4 x the distance of the float32 oracle from the float64 oracle on the same float32 state (H_DIST below, measured
on the CPU, over both energies and every compared chain), at least 4 ulp of max(1, |H|) - the rule of tests/generic_cases.py.
accept[T, C], reject_count and the acceptance rate: exact on every chain inside the row band.  A route without the per-trajectory
outputs is held to rows, cur and reject_count in the same way.

TWO LAUNCHES.  hmc_gauss_wave_kernel carries nothing but the point itself from trajectory to trajectory, so a run cut in two over
traj_offset gives the same bits (asserted).  Every other kernel carries more than `cur` holds - the register-resident direct kernel
d = q - mu and P d, the eigenbasis kernels y = Tin (q - mu) - and rebuilds it from `cur` at the start of a launch: with a non-zero mean
q - mu does not round-trip (tests/test_gpu_hmc.py:test_chunked_launches_equal_single_launch, on a zero mean, states it for the eigenbasis
routes), so there the cut run is compared by value: every decision, reject_count, and the rows inside the row band of the uncut run.
Its energies: up to and including the first trajectory of the second launch both runs start every trajectory from the same float32
point (the cut run rebuilds its representation of it), so H_old and H_new are held to the tolerance of a trajectory-0 energy; from the
next trajectory on the two start points differ by what that rebuild moved (measured 1e-6 .. 3e-6, inside the row band), the tightening to
"the same float32 state" has no ground, and the untightened 10 tol (|H| + 1 + D) holds.

STEP SIZES.  eps = f 2 / omega, omega^2 the largest eigenvalue of M^-1 P (the leapfrog stability limit is f = 1).  Each case's (f, seed)
is the first of f = F_GRID (0.96, 0.92 .. 0.20, then 0.18, 0.16 .. 0.06) x seed = base, base + 1, base + 2 that meets every condition of
tests/test_gauss_traj_cases_cpu.py on the oracle alone (search()); the `tried` column counts the candidates that did not.  No GPU result
entered the choice.

MEASURED on the MI355X when the tests were written (the GPU tests print these figures again; nothing below is a bound).  Per case:
f / oracle acceptance / chains rejecting at burn + 1 of the compared chains, then per route: the larger H_old share of its tolerance /
the larger H_new share / the largest row or cur error of a chain inside the band as a share of the band / chains outside the band
("-": the route has no per-trajectory outputs).  The 489 GPU tests take 6 s.
    r1     0.96/0.32/22 of 31:  small_inline 0.0047/0.059/0.0012/0  small_ws 0.0047/0.059/0.0012/0  eig 0.0047/0.059/0.0012/0
              quad_diag 0.0034/0.059/0.0012/0  quad_two -/-/0.0012/0  general_small 0.0047/0.099/0.00071/0
              small_inline_f64 1.3e-06/1.5e-05/6e-05/0  small_ws_f64 1.3e-06/1.5e-05/6e-05/0  eig_f64 1.3e-06/1.5e-05/6e-05/0
    r2     0.96/0.35/13 of 17:  small_inline 0.023/0.14/0.00055/0  small_ws 0.023/0.14/0.00055/0  eig 0.023/0.35/0.00042/0
              quad_diag 0.027/0.27/0.00042/0  quad_two -/-/0.00042/0  general_small 0.01/0.26/0.0003/0
    r3     0.96/0.23/27 of 31:  small_inline 0.009/0.19/0.0018/0  small_ws 0.009/0.19/0.0018/0  eig 0.013/0.17/0.00099/0
              quad_diag 0.013/0.17/0.00099/0  quad_two -/-/0.00099/0  general_small 0.009/0.24/0.001/0
              small_inline_f64 1e-06/2e-05/2.2e-05/0  small_ws_f64 1e-06/2e-05/2.2e-05/0  eig_f64 3e-06/3.1e-05/2.9e-05/0
              eig_cap 0.013/0.17/0.00099/0  eig_lean -/-/0.00099/0  small_lean -/-/0.0018/0  small_ws_lean -/-/0.0018/0
              small_lean_f64 -/-/2.2e-05/0  eig_lean_f64 -/-/2.9e-05/0
    r4     0.96/0.51/12 of 19:  small_inline 0.034/0.15/0.0018/0  small_ws 0.034/0.15/0.0018/0  eig 0.016/0.26/0.0038/0
              quad_diag 0.031/0.26/0.0038/0  quad_two -/-/0.0038/0  general_small 0.034/0.5/0.0022/0
              small_inline_f64 8.2e-07/8.4e-06/0.0001/0  small_ws_f64 8.2e-07/8.4e-06/0.0001/0  eig_f64 1.9e-06/7.6e-05/0.00028/0
    r5     0.92/0.52/9 of 17:  small_inline 0.087/0.33/0.0013/0  small_ws 0.087/0.33/0.0013/0  eig 0.2/0.33/0.0018/0
              quad_diag 0.2/0.33/0.0018/0  quad_two -/-/0.0018/0  general_small 0.1/0.29/0.00087/0
              wave_eig_f64 2.2e-06/1.3e-05/5.7e-06/0  wave_f64 8.5e-07/2.3e-06/3.1e-06/0
    r6     0.92/0.30/23 of 31:  small_inline 0.049/0.26/0.0013/0  small_ws 0.049/0.26/0.0013/0  eig 0.055/0.3/0.00094/0
              quad_diag 0.055/0.3/0.00094/0  quad_two -/-/0.00094/0  general_small 0.049/0.18/0.0011/0
              wave_eig_f64 4.4e-06/6.7e-05/1.4e-05/0  wave_f64 7.5e-07/6.3e-06/2.2e-06/0  small_lean -/-/0.0013/0
              small_ws_lean -/-/0.0013/0
    w7     0.92/0.24/27 of 31:  wave_eig 0.046/0.11/0.002/0  wave 0.023/0.11/0.0014/0  wave_eig_f64 2.8e-06/2.1e-05/8.2e-06/0
              wave_f64 2.1e-06/2.5e-06/2.7e-06/0
    w63    0.40/0.21/14 of 17:  wave_eig 0.29/0.39/0.0031/0  wave 0.15/0.19/0.00051/0
    w64    0.36/0.35/13 of 17:  wave_eig 0.37/0.38/0.0033/0  wave 0.2/0.27/0.00045/0
    w65    0.60/0.24/14 of 17:  wave_eig 0.59/0.92/0.0063/0  wave 0.2/0.21/0.0015/0
    w127   0.28/0.35/9 of 11:  wave_eig 0.39/0.33/0.0039/0  wave 0.14/0.15/0.00045/0
    w128   0.28/0.35/9 of 11:  wave_eig 0.6/0.67/0.0034/0  wave 0.15/0.2/0.0004/0
    w129   0.28/0.36/8 of 9:  wave_eig 0.19/0.19/0.00056/0  wave 0.19/0.19/0.00056/0
    w99    0.32/0.22/7 of 9:  wave_eig 0.34/0.3/0.0046/0  wave 0.22/0.12/0.00046/0  wave_eig_f64 5.6e-05/6.2e-05/4.4e-05/0
              wave_f64 8.2e-07/1.5e-06/1.8e-06/0
    w100   0.32/0.29/6 of 9:  wave_eig 0.44/0.53/0.004/0  wave 0.21/0.26/0.00038/0  wave_eig_f64 4.9e-05/5.3e-05/4.3e-05/0
              wave_f64 7.8e-07/1.5e-06/1.8e-06/0
    w256   0.20/0.68/4 of 9:  wave 0.22/0.19/0.00048/0
    w257   0.24/0.24/8 of 9:  wave 0.2/0.067/0.00026/0
    w512   0.18/0.25/4 of 5:  wave 0.12/0.23/0.00025/0
    w513   0.18/0.41/6 of 7:  wave 0.13/0.092/0.00032/0
    w1024  0.14/0.70/2 of 5:  wave 0.19/0.12/0.00034/0
    m7f    0.92/0.35/15 of 17:  wave 0.064/0.14/0.00087/0  wave_eig 0.064/0.14/0.00087/0  wave_f64 7e-07/3.5e-06/3.3e-06/0
    m64d   0.44/0.33/8 of 11:  wave 0.24/0.19/0.0005/0  wave_eig 0.24/0.19/0.0005/0
    m65f   0.40/0.30/9 of 11:  wave 0.23/0.18/0.00078/0  wave_eig 0.23/0.18/0.00078/0
    m128d  0.32/0.35/7 of 9:  wave 0.15/0.13/0.0004/0
    m129f  0.32/0.28/8 of 9:  wave 0.16/0.18/0.00072/0
    m256d  0.24/0.54/5 of 9:  wave 0.22/0.2/0.00062/0
    m257f  0.24/0.55/3 of 5:  wave 0.15/0.12/0.00086/0
    m512d  0.20/0.57/4 of 5:  wave 0.11/0.14/0.0003/0
    m513d  0.20/0.33/3 of 5:  wave 0.16/0.076/0.00035/0
    m1024f 0.16/0.55/3 of 5:  wave 0.2/0.15/0.00091/0
    r3d    0.96/0.23/15 of 17:  small_inline 0.0041/0.15/0.00094/0  small_ws 0.0041/0.15/0.00094/0  eig 0.0057/0.08/0.0008/0
              quad_diag 0.0041/0.072/0.0008/0  quad_two -/-/0.0008/0  general_small 0.012/0.16/0.0006/0
              small_inline_f64 5.6e-07/8e-06/1.3e-05/0  eig_f64 2.9e-06/3.5e-05/5.8e-05/0
    r3f    0.96/0.21/15 of 17:  small_inline 0.011/0.24/0.0013/0  small_ws 0.011/0.24/0.0013/0  eig 0.011/0.19/0.002/0
              quad_diag 0.011/0.22/0.002/0  quad_two -/-/0.002/0  general_small 0.011/0.26/0.002/0
              small_inline_f64 1e-06/1.1e-05/3.6e-05/0  eig_f64 1.9e-06/2.6e-05/8e-05/0  small_lean -/-/0.0013/0
              small_lean_f64 -/-/3.6e-05/0
    r6d    0.96/0.24/14 of 17:  small_inline 0.014/0.14/0.0017/0  small_ws 0.014/0.14/0.0017/0  eig 0.014/0.44/0.00099/0
              quad_diag 0.014/0.44/0.00099/0  quad_two -/-/0.00099/0  general_small 0.014/0.36/0.0014/0
    r6f    0.92/0.43/9 of 17:  small_inline 0.091/0.24/0.0022/0  small_ws 0.091/0.24/0.0022/0  eig 0.052/0.67/0.0028/0
              quad_diag 0.052/0.67/0.0028/0  quad_two -/-/0.0028/0  general_small 0.091/0.58/0.002/0
    r3bm1  0.96/0.26/22 of 31:  small_inline 0.009/0.19/0.0018/0  small_ws 0.009/0.19/0.0018/0  eig 0.013/0.17/0.0013/0
              quad_diag 0.013/0.17/0.0013/0  quad_two -/-/0.0013/0  general_small 0.009/0.24/0.001/0
    r3b0   0.96/0.26/23 of 31:  small_inline 0.009/0.19/0.0015/0  small_ws 0.009/0.19/0.0015/0  eig 0.013/0.17/0.0013/0
              quad_diag 0.013/0.17/0.0013/0  quad_two -/-/0.0013/0  general_small 0.009/0.24/0.001/0
    r3b7   0.96/0.26/- of 31:  small_inline 0.009/0.19/0.0032/0  small_ws 0.009/0.19/0.0032/0  eig 0.013/0.17/0.0026/0
              quad_diag 0.013/0.17/0.0026/0  quad_two -/-/0.0026/0  general_small 0.009/0.24/0.002/0
    w7bm1  0.92/0.27/26 of 31:  wave_eig 0.046/0.11/0.0024/0  wave 0.023/0.11/0.0014/0
    w7b0   0.92/0.26/24 of 31:  wave_eig 0.046/0.11/0.0024/0  wave 0.023/0.11/0.0014/0
    w7b7   0.92/0.27/- of 31:  wave_eig 0.046/0.11/0.005/0  wave 0.023/0.11/0.0024/0
    w7c29  0.92/0.25/25 of 29:  wave_eig 0.032/0.11/0.002/0  wave 0.023/0.11/0.0014/0
    w7c30  0.92/0.24/26 of 30:  wave_eig 0.046/0.11/0.002/0  wave 0.023/0.11/0.0014/0
    w7c28  0.92/0.25/24 of 28:  wave_eig 0.032/0.11/0.002/0  wave 0.023/0.11/0.0014/0
    e63    0.96/0.22/47 of 63:  small_inline 0.027/0.34/0.00094/0  small_ws 0.027/0.34/0.00094/0  eig 0.036/0.18/0.00083/0
    e64    0.96/0.23/47 of 64:  small_inline 0.027/0.34/0.00094/0  small_ws 0.027/0.34/0.00094/0  eig 0.036/0.18/0.00084/0
    e65    0.96/0.23/47 of 65:  small_inline 0.027/0.34/0.00094/0  small_ws 0.027/0.34/0.00094/0  eig 0.036/0.18/0.00084/0
              small_cpb 0.027/0.34/0.00094/0
    q15    0.96/0.26/13 of 15:  quad_diag 0.015/0.2/0.0012/0  quad_two -/-/0.0012/0  quad_one -/-/0.0012/0
    q16    0.96/0.27/14 of 16:  quad_diag 0.015/0.2/0.0012/0  quad_two -/-/0.0012/0  quad_one -/-/0.0012/0
    q17    0.96/0.27/14 of 17:  quad_diag 0.015/0.2/0.0012/0  quad_two -/-/0.0012/0  quad_one -/-/0.0012/0
    qo1    0.96/0.32/17 of 24:  quad_one -/-/0.0012/0  quad_two -/-/0.0012/0
    qo2    0.96/0.71/17 of 40:  quad_one -/-/0.0031/0  quad_two -/-/0.0031/0
    qo3    0.96/0.25/20 of 24:  quad_one -/-/0.0012/0  quad_two -/-/0.0012/0
    qo4    0.96/0.24/18 of 24:  quad_one -/-/0.00038/0  quad_two -/-/0.00038/0
    big    0.92/0.33/12 of 17:  wave 0.05/0.18/0.0012/0
Two launches, by value (192 comparisons): H_old / H_new of the cut run against the uncut one at up to 0.97 of the trajectory-0 tolerance up
to the first trajectory of the second launch, at up to 0.002 of the untightened one beyond; rows 1e-6 .. 3e-6 apart.
FOUND AND FIXED by these tests (CHANGELOG): hmc_gauss_quad_kernel<D,true,0> at D <= 3 summed its dummy lane's record slot into both
energies (H_old and H_new 2 log(u)^2 too high, up to 22; their difference, and so every decision, was right); and
hmc_gauss_wave_eig_kernel<float,R> from D = 63 reported both energies 1.5 - 3.0 tolerances low (w63 1.6 / 1.6, w64 1.9 / 2.0, w65 1.5 / 1.7,
w99 2.7 / 2.8, w100 2.5 / 2.5, w127 2.9 / 3.0, w128 3.0 / 3.0 before the fix): the float32 Jacobi eigenvectors came out short,
|v|^2 - 1 = -1e-6, now normalised with their eigenvalues recomputed (eig_polish_kernel, float32 only)."""
import collections
import functools

import numpy as np

import hmc_oracle as O

NTRAJ, BURN, CHAIN_OFFSET = 8, 2, 5
ULP32 = 2.0 ** -23
GUARD = 1e-6               # float64 routes: no decision within GUARD max(1, |H|) of its threshold (tests/mlp_traj_cases.py)
MAX_OUTSIDE = {"f32": 0.05, "f64": 0.0}
MASS_KIND = {"none": 0, "diag": 1, "full": 2}
EIG_ELEMS, QUAD_SLOTS, LDS_BYTES, METRIC_MT = 128, 4, 160 * 1024, 1024          # hmc_gauss_small_dev.hpp, hmc_gauss_quad_dev.hpp, rmhmc_metric_dev.hpp
F_GRID = tuple(round(0.96 - 0.04 * i, 2) for i in range(20)) + tuple(round(0.18 - 0.02 * i, 2) for i in range(7))          # 0.96, 0.92 .. 0.20, 0.18, 0.16 .. 0.06
SEED_BASE = 21

Case = collections.namedtuple("Case", "id D C L mass f seed burn ntraj tried routes")
Route = collections.namedtuple("Route", "keys ws diag f64")

DEFAULT_KEYS = {"gauss_eig": 1, "force_general": 0, "quad_max_chains": 65536, "small_chains_per_block": 0, "quad_variant": 7, "quad_fused": 1}
ROUTES = {
    "small_inline": Route({}, "no", True, False),
    "small_ws": Route({"gauss_eig": 0}, "yes", True, False),
    "small_cpb": Route({"small_chains_per_block": 32}, "no", True, False),
    "eig": Route({"gauss_eig": 2}, "yes", True, False),
    "eig_cap": Route({"quad_max_chains": 8}, "yes", True, False),
    "eig_lean": Route({"gauss_eig": 2}, "yes", False, False),
    "small_lean": Route({}, "no", False, False),
    "small_ws_lean": Route({"gauss_eig": 0}, "yes", False, False),
    "small_lean_f64": Route({}, "no", False, True),
    "eig_lean_f64": Route({}, "yes", False, True),
    "quad_diag": Route({}, "yes", True, False),
    "quad_two": Route({}, "yes", False, False),
    "quad_one": Route({}, "prepared", False, False),
    "wave": Route({"gauss_eig": 0}, "no", True, False),
    "wave_eig": Route({}, "yes", True, False),
    "general_small": Route({"force_general": 1}, "no", True, False),
    "small_inline_f64": Route({}, "no", True, True),
    "small_ws_f64": Route({"gauss_eig": 0}, "yes", True, True),
    "eig_f64": Route({}, "yes", True, True),
    "wave_f64": Route({"gauss_eig": 0}, "no", True, True),
    "wave_eig_f64": Route({}, "yes", True, True),
}
SMALL32 = ("small_inline", "small_ws", "eig", "quad_diag", "quad_two", "general_small")
SMALL64 = ("small_inline_f64", "small_ws_f64", "eig_f64")
WAVE32, WAVE64 = ("wave_eig", "wave"), ("wave_eig_f64", "wave_f64")
LEAN = ("small_lean", "small_ws_lean", "small_lean_f64", "eig_lean_f64")          # no per-trajectory outputs: what a plain sample() launches

# id, D, chains, L, mass, burn, routes.  (f, seed, tried) of every case: STEPS, filled by search().
_SPEC = [
    # 1 / 2: the register-resident kernels, float32 D = 1 .. 6, float64 D = 1, 3, 4
    ("r1", 1, 31, 3, "none", BURN, SMALL32 + SMALL64),
    ("r2", 2, 17, 2, "none", BURN, SMALL32),
    ("r3", 3, 31, 3, "none", BURN, SMALL32 + SMALL64 + ("eig_cap", "eig_lean") + LEAN),
    ("r4", 4, 19, 5, "none", BURN, SMALL32 + SMALL64),
    ("r5", 5, 17, 4, "none", BURN, SMALL32 + WAVE64),          # 4: float64 D = 5 is the first wave-kernel size
    ("r6", 6, 31, 3, "none", BURN, SMALL32 + WAVE64 + ("small_lean", "small_ws_lean")),
    # 3: the wave kernels, identity mass: D = 7 .. 129 (129 leaves the eigenbasis route)
    ("w7", 7, 31, 3, "none", BURN, WAVE32 + WAVE64),
    ("w63", 63, 17, 2, "none", BURN, WAVE32),
    ("w64", 64, 17, 2, "none", BURN, WAVE32),
    ("w65", 65, 17, 3, "none", BURN, WAVE32),
    ("w127", 127, 11, 2, "none", BURN, WAVE32),
    ("w128", 128, 11, 2, "none", BURN, WAVE32),
    ("w129", 129, 9, 2, "none", BURN, WAVE32),
    # 4: float64 D = 99 | 100: the diagonalisation moves into the workspace slab
    ("w99", 99, 9, 2, "none", BURN, WAVE32 + WAVE64),
    ("w100", 100, 9, 2, "none", BURN, WAVE32 + WAVE64),
    # 5: the direct wave kernel by R (64 | 65, 128 | 129 above), every R with an identity, a diagonal and a dense mass
    ("w256", 256, 9, 2, "none", BURN, ("wave",)),
    ("w257", 257, 9, 2, "none", BURN, ("wave",)),
    ("w512", 512, 5, 2, "none", BURN, ("wave",)),
    ("w513", 513, 7, 2, "none", BURN, ("wave",)),
    ("w1024", 1024, 5, 2, "none", BURN, ("wave",)),
    ("m7f", 7, 17, 3, "full", BURN, ("wave", "wave_eig", "wave_f64")),          # (a dense mass refuses the eigenbasis route)
    ("m64d", 64, 11, 2, "diag", BURN, ("wave", "wave_eig")),
    ("m65f", 65, 11, 2, "full", BURN, ("wave", "wave_eig")),
    ("m128d", 128, 9, 2, "diag", BURN, ("wave",)),
    ("m129f", 129, 9, 2, "full", BURN, ("wave",)),
    ("m256d", 256, 9, 2, "diag", BURN, ("wave",)),
    ("m257f", 257, 5, 2, "full", BURN, ("wave",)),
    ("m512d", 512, 5, 2, "diag", BURN, ("wave",)),
    ("m513d", 513, 5, 2, "diag", BURN, ("wave",)),
    ("m1024f", 1024, 5, 2, "full", BURN, ("wave",)),
    # 6: mass kinds on the quad / eig / small routes (the eigen routes whiten the mass: Tin, Tout, Qt)
    ("r3d", 3, 17, 3, "diag", BURN, SMALL32 + ("small_inline_f64", "eig_f64")),
    ("r3f", 3, 17, 3, "full", BURN, SMALL32 + ("small_inline_f64", "eig_f64", "small_lean", "small_lean_f64")),
    ("r6d", 6, 17, 3, "diag", BURN, SMALL32),
    ("r6f", 6, 17, 3, "full", BURN, SMALL32),
    # 7: burn -1, 0 and T - 1 (2: r3, w7)
    ("r3bm1", 3, 31, 3, "none", -1, SMALL32),
    ("r3b0", 3, 31, 3, "none", 0, SMALL32),
    ("r3b7", 3, 31, 3, "none", NTRAJ - 1, SMALL32),
    ("w7bm1", 7, 31, 3, "none", -1, WAVE32),
    ("w7b0", 7, 31, 3, "none", 0, WAVE32),
    ("w7b7", 7, 31, 3, "none", NTRAJ - 1, WAVE32),
    # 8: the wave kernels' launch edge, 4 chains per block: C % 4 = 1, 2, 0 (3: w7)
    ("w7c29", 7, 29, 3, "none", BURN, WAVE32),
    ("w7c30", 7, 30, 3, "none", BURN, WAVE32),
    ("w7c28", 7, 28, 3, "none", BURN, WAVE32),
    # 9: the small and eig kernels' launch edge, 64 chains per block (and 32 once: small_chains_per_block)
    ("e63", 5, 63, 2, "none", BURN, ("small_inline", "small_ws", "eig")),
    ("e64", 5, 64, 2, "none", BURN, ("small_inline", "small_ws", "eig")),
    ("e65", 5, 65, 2, "none", BURN, ("small_inline", "small_ws", "eig", "small_cpb")),
    # 10: the quad kernel's launch edge, 16 chains per wave
    ("q15", 3, 15, 3, "none", BURN, ("quad_diag", "quad_two", "quad_one")),
    ("q16", 3, 16, 3, "none", BURN, ("quad_diag", "quad_two", "quad_one")),
    ("q17", 3, 17, 3, "none", BURN, ("quad_diag", "quad_two", "quad_one")),
    # the one-launch quad route at its defaults: C % 8 == 0
    ("qo1", 1, 24, 3, "none", BURN, ("quad_one", "quad_two")),
    ("qo2", 2, 40, 5, "none", BURN, ("quad_one", "quad_two")),
    ("qo3", 3, 24, 3, "none", BURN, ("quad_one", "quad_two")),
    ("qo4", 4, 24, 2, "none", BURN, ("quad_one", "quad_two")),
]
BIG_C = 4 * 65535 + 1          # 8: one launch of more than 65 535 workgroups of the wave kernel, compared on 17 probe chains
_SPEC.append(("big", 7, BIG_C, 3, "none", BURN, ("wave",)))

# id -> (f, seed, tried): the output of search() (python tests/test_gauss_traj_cases_cpu.py)
STEPS = {
    'r1': (0.96, 21, 0),
    'r2': (0.96, 21, 0),
    'r3': (0.96, 21, 0),
    'r4': (0.96, 21, 0),
    'r5': (0.92, 21, 3),
    'r6': (0.92, 21, 3),
    'w7': (0.92, 21, 3),
    'w63': (0.4, 22, 43),
    'w64': (0.36, 21, 45),
    'w65': (0.6, 21, 27),
    'w127': (0.28, 21, 51),
    'w128': (0.28, 21, 51),
    'w129': (0.28, 21, 51),
    'w99': (0.32, 22, 49),
    'w100': (0.32, 22, 49),
    'w256': (0.2, 21, 57),
    'w257': (0.24, 23, 56),
    'w512': (0.18, 22, 61),
    'w513': (0.18, 21, 60),
    'w1024': (0.14, 21, 66),
    'm7f': (0.92, 21, 3),
    'm64d': (0.44, 21, 39),
    'm65f': (0.4, 21, 42),
    'm128d': (0.32, 21, 48),
    'm129f': (0.32, 21, 48),
    'm256d': (0.24, 21, 54),
    'm257f': (0.24, 21, 54),
    'm512d': (0.2, 21, 57),
    'm513d': (0.2, 22, 58),
    'm1024f': (0.16, 21, 63),
    'r3d': (0.96, 21, 0),
    'r3f': (0.96, 21, 0),
    'r6d': (0.96, 21, 0),
    'r6f': (0.92, 21, 3),
    'r3bm1': (0.96, 21, 0),
    'r3b0': (0.96, 21, 0),
    'r3b7': (0.96, 21, 0),
    'w7bm1': (0.92, 21, 3),
    'w7b0': (0.92, 21, 3),
    'w7b7': (0.92, 21, 3),
    'w7c29': (0.92, 21, 3),
    'w7c30': (0.92, 21, 3),
    'w7c28': (0.92, 21, 3),
    'e63': (0.96, 22, 1),
    'e64': (0.96, 22, 1),
    'e65': (0.96, 22, 1),
    'q15': (0.96, 21, 0),
    'q16': (0.96, 21, 0),
    'q17': (0.96, 21, 0),
    'qo1': (0.96, 21, 0),
    'qo2': (0.96, 21, 0),
    'qo3': (0.96, 21, 0),
    'qo4': (0.96, 21, 0),
    'big': (0.92, 21, 3),
}

# id -> the largest |H(float32 oracle) - H(float64 oracle)| of trajectory 0 over H_old, H_new and the compared chains, rounded up to two
# digits (measured again by tests/test_gauss_traj_cases_cpu.py)
H_DIST = {
    'r1': 8.7e-06,
    'r2': 3.2e-06,
    'r3': 1.3e-05,
    'r4': 4.7e-06,
    'r5': 1.2e-06,
    'r6': 3.5e-06,
    'w7': 6.6e-06,
    'w63': 8.2e-06,
    'w64': 5.2e-06,
    'w65': 4.4e-06,
    'w127': 1.3e-05,
    'w128': 8.1e-06,
    'w129': 7.5e-06,
    'w99': 7.5e-06,
    'w100': 8.1e-06,
    'w256': 2.2e-05,
    'w257': 1.7e-05,
    'w512': 3e-05,
    'w513': 2.6e-05,
    'w1024': 4.1e-05,
    'm7f': 3.3e-06,
    'm64d': 5.9e-06,
    'm65f': 5.7e-06,
    'm128d': 1.2e-05,
    'm129f': 4.9e-06,
    'm256d': 1.3e-05,
    'm257f': 1.4e-05,
    'm512d': 3.6e-05,
    'm513d': 2.8e-05,
    'm1024f': 6.3e-05,
    'r3d': 1.4e-05,
    'r3f': 1.1e-05,
    'r6d': 8.3e-06,
    'r6f': 2.3e-06,
    'r3bm1': 1.3e-05,
    'r3b0': 1.3e-05,
    'r3b7': 1.3e-05,
    'w7bm1': 6.6e-06,
    'w7b0': 6.6e-06,
    'w7b7': 6.6e-06,
    'w7c29': 6.6e-06,
    'w7c30': 6.6e-06,
    'w7c28': 6.6e-06,
    'e63': 8.3e-06,
    'e64': 8.3e-06,
    'e65': 8.3e-06,
    'q15': 1.1e-05,
    'q16': 1.1e-05,
    'q17': 1.1e-05,
    'qo1': 6.7e-06,
    'qo2': 8.6e-06,
    'qo3': 1.1e-05,
    'qo4': 8.6e-06,
    'big': 4.8e-06,
}


def _build_table():
    out = []
    for id_, D, C, L, mass, burn, routes in _SPEC:
        f, seed, tried = STEPS.get(id_, (None, SEED_BASE, 0))
        out.append(Case(id_, D, C, L, mass, f, seed, burn, NTRAJ, tried, tuple(routes)))
    return out


TABLE = _build_table()
CASES = {c.id: c for c in TABLE}
CUT_IDS = ("r3", "r3f", "r6", "r4", "w7", "w65", "w129", "m7f", "m65f", "q16", "qo3", "w99")          # two launches over traj_offset
PAD_IDS = ("r3", "r6f", "w7", "w65", "m7f", "q17", "qo3", "w257")                                      # rows behind the last chain


def tag(route):
    return "f64" if ROUTES[route].f64 else "f32"


def probe_chains(case):
    """The chains of a case that go against the oracle: all, or for the big launch the first 4, the last 4 and 9 spread between."""
    if case.C <= 4096:
        return np.arange(case.C)
    mid = np.round(np.linspace(4, case.C - 5, 11)[1:-1]).astype(np.int64)
    sel = np.concatenate([np.arange(4), mid, np.arange(case.C - 4, case.C)])
    assert sel.size == 17 and len(set(sel.tolist())) == 17
    return sel


# ---- the launcher's rules, restated ----
def metric_slab_bytes(D, elem):
    """rmhmc_metric.hip:metric_geometry for one system of D <= 128: the bytes of the global slab its diagonalisation needs (0 while
    both matrices fit one CU's LDS: float32 throughout, float64 up to D = 99)."""
    assert D <= 128
    ne, vn = D + (D & 1), 16 // elem
    ldv = (D + vn - 1) // vn * vn
    size = lambda lda, ldv_: (ne * lda + D * ldv_ + 5 * ne + 4 + METRIC_MT // 64) * elem + ne * 4 + 64
    lds = size(ne + 1, ldv) if size(ne + 1, ldv) <= LDS_BYTES else size(ne, ldv)
    vglobal = lds > LDS_BYTES
    if vglobal:
        lds = size(ne + 1, 0) if size(ne + 1, 0) <= LDS_BYTES else size(ne, 0)
    NP, nv = ne // 2, ldv // vn
    mid = NP * (NP + 1) // 2 <= 4 * METRIC_MT and NP * nv <= 3 * METRIC_MT
    if lds > LDS_BYTES or not mid or (vglobal and elem == 8):
        return ((D * ldv + ne * (ne + 1) + 3) & ~3) * elem
    return D * ldv * elem if vglobal else 0


def workspace_bytes(C, D, n_traj, elem):
    """hta_hmc_gaussian_workspace_bytes."""
    if D > 6:
        area = ((2 * D * D + D + 64) * elem + 15) & ~15
        return area + (metric_slab_bytes(D, elem) if D <= 128 else 0)
    per_vec = 16 // elem
    rec = (D + 1 + per_vec - 1) // per_vec * per_vec
    return (n_traj + QUAD_SLOTS) * C * rec * elem + EIG_ELEMS * elem


def wave_r(D):
    R = (D + 63) // 64
    return next(r for r in (1, 2, 4, 8, 16) if R <= r)


def expected_route(case, route, n_traj=None):
    """gaussian_dispatch / launch_small / quad_route / quad_fused_route / wave_eig_route under the keys, the workspace and the outputs
    of `route`: the string _abi.last_route() must report for a launch of n_traj trajectories (default: the case's; a prepared
    workspace is prepared for the case's count)."""
    r = ROUTES[route]
    k = dict(DEFAULT_KEYS, **r.keys)
    D, C, L, kind = case.D, case.C, case.L, MASS_KIND[case.mass]
    n = case.ntraj if n_traj is None else n_traj
    T = "double" if r.f64 else "float"
    b = lambda x: "true" if x else "false"
    ws_z = r.ws != "no" and D <= 6
    ws_logu = r.ws != "no" and bool(k["gauss_eig"])
    reg = D <= (4 if r.f64 else 6) and not k["force_general"]
    if not (ws_z and reg):
        ws_z = False
        ws_logu = ws_logu and not reg
    if reg:
        if ws_z and ws_logu:
            if not r.f64 and D <= 4 and k["gauss_eig"] != 2 and C <= k["quad_max_chains"] and C <= 1 << 24:
                lb = 0 if k["gauss_eig"] == 3 else L
                lbv = lb if lb in (25, 10, 5) else 0
                W = (D + 1 + 3) // 4 * 4
                if (k["quad_fused"] and not r.diag and k["quad_variant"] == 7 and C <= 4096 and n >= 8 and (C * W * 4) % 128 == 0
                        and r.ws == "prepared" and n == case.ntraj):
                    return "hmc_gauss_quad_fused_kernel<%d,%d>" % (D, lbv)
                if not r.diag and k["quad_variant"] in (3, 7) and C <= 1 << 20:
                    return "hmc_gauss_quad_kernel<%d,false,%d,%d>" % (D, lbv, k["quad_variant"])
                return "hmc_gauss_quad_kernel<%d,%s,%d>" % (D, b(r.diag), 0 if r.diag else lbv)
            return "hmc_gauss_eig_kernel<%s,%d,%s>" % (T, D, b(r.diag))
        return "hmc_gauss_small_kernel<%s,%d,%d,%s,%s>" % (T, D, kind, b(ws_z), b(r.diag))
    if kind == 0 and ws_logu and D <= 128:
        return "hmc_gauss_wave_eig_kernel<%s,%d>" % (T, min(wave_r(D), 2))
    return "hmc_gauss_wave_kernel<%s,%d,%d>" % (T, wave_r(D), kind)


def is_wave(name):
    return name.startswith("hmc_gauss_wave")


def carries_only_the_point(name):
    """TWO LAUNCHES above: the kernels whose cut run repeats the uncut run's bits."""
    return name.startswith("hmc_gauss_wave_kernel")


def runs():
    """Every (case id, route) of the table.  A route that refuses a case is run all the same: expected_route says where it lands."""
    return [(c.id, r) for c in TABLE for r in c.routes]


# ---- inputs and the oracle ----
def log_norm(D):
    return -1.0 - 0.25 * D


def _rand_spd(D, seed, lo, hi):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    P = (Q * np.linspace(lo, hi, D)) @ Q.T
    return 0.5 * (P + P.T)


@functools.lru_cache(maxsize=None)
def inputs_of(D):
    """(P[D, D], mu[D]) in float32, read-only (tests/rmhmc_traj_cases.py:inputs_of)."""
    P = _rand_spd(D, 1000 + D, 0.5, 2.0).astype(np.float32)
    P = 0.5 * (P + P.T)
    mu = np.linspace(-1.0, 1.0, D).astype(np.float32)
    P.setflags(write=False); mu.setflags(write=False)
    return P, mu


@functools.lru_cache(maxsize=None)
def inv_mass_of(D, mass):
    """tests/test_gpu_hmc.py:masses in float32: None, a diagonal [D] or a symmetric [D, D]; read-only."""
    if mass == "none":
        return None
    rng = np.random.default_rng(0)
    diag = rng.uniform(0.5, 2.0, D)
    if mass == "diag":
        im = diag.astype(np.float32)
    else:
        im = _rand_spd(D, 7, 0.5, 1.5).astype(np.float32)
        im = 0.5 * (im + im.T)
    im.setflags(write=False)
    return im


def mass_operands(case, dtype):
    """(mass kind, inv_mass, mass_factor) as hamiltorch_amd/samplers.py:_mass_operands hands them to the kernels, from the float32
    inv_mass in float64, rounded to `dtype`: diag sqrt(1 / inv_mass), full chol(inverse(inv_mass))."""
    im = inv_mass_of(case.D, case.mass)
    if im is None:
        return 0, None, None
    im64 = im.astype(np.float64)
    mf = np.sqrt(1.0 / im64) if im.ndim == 1 else np.linalg.cholesky(np.linalg.inv(im64))
    return MASS_KIND[case.mass], im.astype(dtype), mf.astype(dtype)


@functools.lru_cache(maxsize=None)
def omega_max(D, mass):
    """sqrt of the largest eigenvalue of M^-1 P: the leapfrog is stable for eps < 2 / omega."""
    P = inputs_of(D)[0].astype(np.float64)
    im = inv_mass_of(D, mass)
    A = P if im is None else (im.astype(np.float64)[:, None] * P if im.ndim == 1 else im.astype(np.float64) @ P)
    return float(np.sqrt(np.abs(np.linalg.eigvals(A)).max()))


def eps_of(case):
    """The step size as every launch and the oracle take it: f 2 / omega rounded to float32."""
    return float(np.float32(case.f * 2.0 / omega_max(case.D, case.mass)))


def starts(case, chains=None):
    """theta_init of the chains `chains` (default: all) in float32: mu + 0.3 z, z the Philox INIT normals of (seed, chain id)."""
    chains = np.arange(case.C) if chains is None else np.asarray(chains)
    mu = inputs_of(case.D)[1].astype(np.float64)
    z = O.philox_normals(case.seed, CHAIN_OFFSET + chains, 0, case.D, O.PURPOSE_INIT, dtype=np.float64)
    return (mu + 0.3 * z).astype(np.float32)


class _Recording(O.GaussianTarget):
    """hmc_hamiltonian asks for log p once: at a trajectory's start, then at its end."""

    def __init__(self, mu, P, log_norm):
        super().__init__(mu, P, log_norm)
        self.seen = []

    def logp(self, theta):
        self.seen.append(np.array(theta, copy=True))
        return super().logp(theta)


class _RestartedDraws(O.PhiloxDraws):
    """A wrong kernel's draws: the second of two launches cut at n0 indexes its draws by t instead of traj_offset + t."""

    def __init__(self, seed, chain_ids, dtype, n0):
        super().__init__(seed, chain_ids, dtype)
        self.n0 = n0

    def normals(self, n, D, sub=0):
        return super().normals(n - self.n0 if n >= self.n0 else n, D, sub)

    def mh_uniform(self, n):
        return super().mh_uniform(n - self.n0 if n >= self.n0 else n)


Ref = collections.namedtuple("Ref", "rows h_old h_new accept rejected acc_rate log_u starts cur theta0")


def run_oracle(case, chains=None, dtype=np.float64, mean="case", lognorm="case", mass="case", ntraj=None, restart_at=None):
    """sample_hmc on the chains `chains` of the case (default: probe_chains), state and draws in `dtype`, from the float32 inputs.
    Ref: rows[T - burn, c, D] (row 0 = theta_init), h_old / h_new / accept[T, c], rejected[c], acc_rate[c], log_u[T, c] (float64),
    starts[T, c, D] (the point every trajectory starts from), cur[c, D] (the state after the last trajectory), theta0[c, D].
    mean=None: the target's mean at 0 (the starts stay); lognorm=None: log_norm 0; mass=None: identity mass; ntraj: only the first
    trajectories; restart_at: _RestartedDraws."""
    P, mu = inputs_of(case.D)
    chains = probe_chains(case) if chains is None else np.asarray(chains)
    ids = CHAIN_OFFSET + chains
    th0 = starts(case, chains)
    n = case.ntraj if ntraj is None else ntraj
    burn = min(case.burn, n - 1)
    tg = _Recording((mu if mean == "case" else np.zeros_like(mu)).astype(dtype), P.astype(dtype), log_norm(case.D) if lognorm == "case" else 0.0)
    im = inv_mass_of(case.D, case.mass) if mass == "case" else None
    draws = O.PhiloxDraws(case.seed, ids, dtype) if restart_at is None else _RestartedDraws(case.seed, ids, dtype, restart_at)
    ret, info = O.sample_hmc(tg, th0.astype(dtype), n, case.L, dtype(eps_of(case)), burn, None if im is None else im.astype(dtype), draws)
    assert len(tg.seen) == 2 * n
    acc = np.stack(info["accept"])
    ho, hn = np.stack(info["h_old"]), np.stack(info["h_new"])
    log_u = np.stack([np.log(O.PhiloxDraws(case.seed, ids, np.float64).mh_uniform(k).astype(np.float64)) for k in range(n)])
    begin = np.stack(tg.seen[0::2])
    last = n - 1
    kept = th0.astype(dtype) if last == burn + 1 else begin[last]
    cur = np.where(acc[last][:, None], tg.seen[-1], kept)
    return Ref(np.stack(ret), ho, hn, acc, (~acc).sum(0), info["acc_rate"], log_u, begin, cur, th0)


def _frozen(ref):
    for a in ref:
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(cid):
    """The float64 oracle of a case on its probe chains; computed once per process, shared by every test that needs it, read-only."""
    return _frozen(run_oracle(CASES[cid]))


# ---- the bounds ----
def row_tol(tag_, name, D):
    if tag_ == "f64":
        return 1e-9 if is_wave(name) else 1e-10
    return 5e-4 if D >= 257 else 3e-4 if is_wave(name) else 2e-4


def row_band(tag_, name, D, want):
    return row_tol(tag_, name, D) * (max(1.0, float(np.abs(want).max())) if tag_ == "f32" else 1.0)


def h_tol(tag_, case, H, dist=None):
    """The tolerance of a trajectory-0 energy (BOUNDS above); dist: in place of the recorded H_DIST (the search's candidates)."""
    loose = 10.0 * (2e-5 if tag_ == "f32" else 1e-11) * (np.abs(H) + 1.0 + case.D)
    if tag_ == "f64":
        return loose
    return np.minimum(loose, np.maximum(4.0 * (H_DIST[case.id] if dist is None else dist), 4.0 * ULP32 * np.maximum(1.0, np.abs(H))))


def h_tol_loose(tag_, case, H):
    """The tolerance of an energy whose two sides did not start from the same float32 state: 10 tol (|H| + 1 + D), untightened."""
    return 10.0 * (2e-5 if tag_ == "f32" else 1e-11) * (np.abs(H) + 1.0 + case.D)


def max_outside(tag_, n_chains):
    """Chains allowed outside the row band: 5 % of the compared ones in float32, none in float64."""
    return int(MAX_OUTSIDE[tag_] * n_chains)


def outside(rows, cur, ref, band):
    """Chain by chain: True where any entry of any row of the chain, or of the state handed back, is further than `band`."""
    assert rows.shape == ref.rows.shape and cur.shape == ref.cur.shape, (rows.shape, ref.rows.shape)
    with np.errstate(invalid="ignore"):
        return ~((np.abs(rows - ref.rows).max(axis=(0, 2)) <= band) & (np.abs(cur - ref.cur).max(axis=1) <= band))


def guard_margin(ref):
    """|min(0, H_old - H_new) - log u| / max(1, |H_old|, |H_new|): the distance of a Metropolis decision from its threshold."""
    scale = np.maximum(1.0, np.maximum(np.abs(ref.h_old), np.abs(ref.h_new)))
    return np.abs(np.minimum(0.0, ref.h_old - ref.h_new) - ref.log_u) / scale


def h_distance(case):
    """max |H(float32 oracle) - H(float64 oracle)| over both energies of trajectory 0 and the compared chains."""
    a, b = run_oracle(case, ntraj=1), run_oracle(case, dtype=np.float32, ntraj=1)
    return float(max(np.abs(a.h_old[0] - b.h_old[0]).max(), np.abs(a.h_new[0] - b.h_new[0]).max()))


def search(spec_id, check):
    """The first (f, seed) of F_GRID x (SEED_BASE, + 1, + 2) for which check(case) raises no AssertionError: (f, seed, tried)."""
    c = CASES[spec_id]
    tried = 0
    for f in F_GRID:
        for seed in range(SEED_BASE, SEED_BASE + 3):
            cand = c._replace(f=f, seed=seed)
            try:
                check(cand)
                return f, seed, tried
            except AssertionError:
                tried += 1
    raise RuntimeError("no candidate of the grid serves %s" % spec_id)
