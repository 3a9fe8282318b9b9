#define HTA_PHILOX_MAD64 1      // philox.hpp: 64-bit products (this file's kernels have the registers for them)
// Explicit RMHMC for a Gaussian target on the identity-soft-abs path (rmhmc_fused.hip: why that path exists; the integrator is
// hamiltorch/samplers.py:425-461 inside the sampler loop S:969-1026), ONE chain per four-wave workgroup: the kernel of BASELINE
// config 3 (256 chains on 256 CUs).  Round 4: the third generation of rmhmc_uv_kernel<1>, built from what ablation builds of
// that kernel measured (profiles/r04b_uv_ablation.txt; per step at 256 chains: 1.01 us in the 312 matrix instructions, 0.65 us in
// the five LDS publish / barrier / fetch round trips, 0.94 us issuing the ~570 other instructions of a lone wave):
//
// (1) COMPACT ELEMENT-WISE LAYOUT.  The product leaves four rows per lane, twice over (both contraction parities) and in four
//     columns of which one chain fills two (its state set U = (theta, p) and the copy V = (theta_c, p_c), S:425-426): the
//     element-wise work of rmhmc_uv_kernel<1> ran every instruction four times for one useful value in four.  Here the eight
//     lanes of a row block (4 columns x 2 parities) split its 4 rows x 2 sets: lane (column cl, parity kp) OWNS row
//     row0 + 2 (cl >> 1) + kp of set cl & 1 - one value per lane, every element-wise instruction once, every lane useful.  Going
//     from the accumulator to that layout costs four selects, two DPP adds (the parity sum, needed anyway) and one select with a
//     quad permutation.
// (2) THREE PRODUCT PHASES PER STEP INSTEAD OF FIVE.  A half step solves x = (P + E)^-1 g, E = diag(jitter u), by K = 2
//     refinements from x0 = z = S g (S = P^-1 shared): x2 = z - S(e . (z - S(e . z))) = z - r1 + c2, r1 = S(e . z), c2 = S(e . r1).
//     c2 is second order in rho = jitter / lambda_min (cfg3: 2e-3): it only has to be ADDED to theta, and products that take a
//     vector carrying c2 as input change by third-order terms - below the rounding the host picked K for (rho^(K+1) <= eps / 4).
//     So a solve is ONE phase (r1), and c2 = S q, q = e . r1, rides in the two idle columns of the NEXT phase's instruction (a
//     one-chain group leaves columns 2, 3 of v_mfma_f32_4x4x1_16b free); when it arrives it is added where theta entered since
//     (z -= eh (theta - mu): a multiple of c2; the rotation S:447-450 is linear: its image of (c2_U, c2_V) is added to the rotated
//     state; P c2 = q needs no product; the momentum part of that image goes through S once more, again in idle columns).
//     Per step: phase 1 (A pair: r1, and c2 of the previous B pair), phase 2 (after the rotation: y = P (theta - mu), z = S p
//     afresh, and c2 of the A pair), phase 3 (B pair: r1, and S of the rotation's momentum correction) - 208 matrix instructions
//     and three barriers instead of 312 and five; one flush phase per trajectory.  The result equals the K = 2 iteration up to
//     third-order terms (oracle/ prototype: identical error against the exact solve, 1.9e-9 in float64 at cfg3's sizes).
// Everything else is the trajectory shell of rmhmc_cols_dev.hpp (cols_trajectories), shared with rmhmc_uv_kernel: same Philox
// streams, same update order, momenta drawn ahead, the V column of a trajectory's last Hamiltonian evaluates the next
// trajectory's momentum terms.  UvcTile holds the layout, steps() and hamiltonian() of this kernel.  Only launched for K == 2 with
// jitter; anything else stays on rmhmc_uv_kernel.
#include <math.h>
#include "rmhmc_cols_dev.hpp"

namespace hta {

struct UvcTile : ColsLane {
  static constexpr int NV = 1, NC = 1, cidx = 0, NBUF = 7;       // (NBUF) LDS vector matrices: DV GV EV W0 W1 WA WB
  T *WA, *WB, *red;                // A pair: e . z | q of the previous B pair; B pair: e . z | the rotation's momentum correction; [XWV][2][4]
  int own_off, def_off, row[1];                           // GV's columns 2, 3 (def_off): the A pair's q
  bool rok[1], rok_p, hih, writer, row_writer;
  T mu_r[1], sd_r[1], ehU, ehV, zc2, kXo, kXp, kGo, kGp;

  __device__ __forceinline__ UvcTile(const FusedArgs<float>& a_, T* lds) : ColsLane(a_, lds) {
    WA = W0 + 2 * MSZ; WB = WA + MSZ; red = WB + MSZ;
    hih = (cl >> 1) != 0;
    writer = tid == 0; row_writer = !setV;
    row[0] = row0 + 2 * (cl >> 1) + kpar;                 // this lane OWNS row row[0] of set cl & 1
    rok[0] = row[0] < a.D; rok_p = (row[0] ^ 1) < a.D;    // (row ^ 1: the row of the lane at the other parity)
    mu_r[0] = rok[0] ? a.mu[row[0]] : 0.f;
    sd_r[0] = rok[0] ? a.S[(int64_t)row[0] * a.D + row[0]] : 0.f;
    zero_lds(NBUF * MSZ + XWV * 2 * 4);
    ehU = setV ? 0.f : eh; ehV = setV ? eh : 0.f;         // the set that moves first in S:429-433 is U, in S:454-458 V
    zc2 = setV ? 0.f : -2.f * eh * eh;                    // what z_U misses while c2 of a B pair is in flight (two kicks: S:458, S:429)
    // the rotation S:447-450 as a linear map of (d theta, 0, d theta_c, 0) (sequential, Q1): this set's rows of it
    const T hc = 0.5f, rc = a.rot_c, rs = a.rot_s;
    const T t_u = hc * (1.f + rc), t_v = hc * (1.f - rc);                                   // theta'   = t_u du + t_v dv
    const T p_u = -hc * rs * t_u, p_v = -hc * rs * (t_v - 1.f);                             // p'       = -s/2 (theta' - dv)
    const T c_u = hc * (t_u - rc * t_u - rs * p_u), c_v = hc * ((t_v + 1.f) - rc * (t_v - 1.f) - rs * p_v);   // theta_c'
    const T q_u = hc * (p_u + rs * (t_u - c_u) - rc * p_u), q_v = hc * (p_v + rs * (t_v - c_v) - rc * p_v);   // p_c'
    // this lane's coefficients on (own c2, partner's c2), eh folded in: X and g corrections
    kXo = eh * (setV ? c_v : t_u); kXp = eh * (setV ? c_u : t_v);
    kGo = eh * (setV ? q_v : p_u); kGp = eh * (setV ? q_u : p_v);
    own_off = (cl & 1) * XLD + (row[0] & 1) * XHL + (row[0] >> 1); def_off = own_off + 2 * XLD;
  }
  __device__ __forceinline__ void put(T* X, const T (&v)[1]) const { X[own_off] = v[0]; }
  // the owned value of (set cl & 1) out of the instruction's columns 0 / 1, and that of columns 2 / 3 (the deferred products)
  __device__ __forceinline__ void extract2(const bf4& acc, T& main, T& defer) const {
    const T m01 = khi ? acc[1] : acc[0], o01 = khi ? acc[0] : acc[1];
    const T m23 = khi ? acc[3] : acc[2], o23 = khi ? acc[2] : acc[3];
    const T s01 = m01 + other_parity(o01), s23 = m23 + other_parity(o23);   // rows row0 + kp, row0 + 2 + kp of THIS lane's column
    // (the cross-lane reads stand OUTSIDE the selects: inside an arm they would run under that arm's lane mask)
    const T lo23 = quad_dpp<0x44>(s23);                    // [0,1,0,1]: columns 2, 3 take the rows 2 + kp of columns 0, 1
    const T hi01 = quad_dpp<0xEE>(s01);                    // [2,3,2,3]: columns 0, 1 take the rows kp of columns 2, 3
    main = hih ? lo23 : s01;
    defer = hih ? s23 : hi01;
  }
  __device__ __forceinline__ void extract(const bf4& acc, T (&v)[1]) const {
    const T m01 = khi ? acc[1] : acc[0], o01 = khi ? acc[0] : acc[1];
    const T m23 = khi ? acc[3] : acc[2], o23 = khi ? acc[2] : acc[3];
    const T s01 = m01 + other_parity(o01), s23 = m23 + other_parity(o23);
    const T lo23 = quad_dpp<0x44>(s23);
    v[0] = hih ? lo23 : s01;
  }
  // this lane's element of one jitter vector (uniform_elem layout: rows 4b..4b+3 are Philox block b)
  __device__ __forceinline__ void jitter_one(uint32_t n, uint32_t sub, T (&e)[1]) const {
    const U4 r = philox_block(a.seed, chain, n, PURPOSE_JITTER, sub, (uint32_t)(row0 >> 2));
    const uint32_t t0 = hih ? r.z : r.x, t1 = hih ? r.w : r.y;
    e[0] = (live && rok[0]) ? a.jitter * u23<T>(khi ? t1 : t0) : 0.f;
  }
  // the two jitter vectors of a step's solves for this set (sub-streams subA, subB): the even parity draws the block of the A
  // pair, the odd parity that of the B pair, each hands the other the element of the other's row - one Philox pass per step
  __device__ __forceinline__ void jitter_pair(uint32_t n, uint32_t subA, uint32_t subB, T& eA, T& eB) const {
    const U4 r = philox_block(a.seed, chain, n, PURPOSE_JITTER, khi ? subB : subA, (uint32_t)(row0 >> 2));
    const uint32_t t0 = hih ? r.z : r.x, t1 = hih ? r.w : r.y;
    const T mine = (live && rok[0]) ? a.jitter * u23<T>(khi ? t1 : t0) : 0.f;
    const T oth = other_parity((live && rok_p) ? a.jitter * u23<T>(khi ? t0 : t1) : 0.f);
    eA = khi ? oth : mine;
    eB = khi ? mine : oth;
  }
  // three sums per set over the rows, complete in every lane of the set
  __device__ __forceinline__ void sums(T (&v)[3]) const {
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      v[e] += quad_dpp<0x4E>(v[e]);                        // [2,3,0,1]: the same set's other row pair
      v[e] += quad_dpp<0x124>(v[e]);                       // row_ror:4
      v[e] += other_parity(v[e]);                          // row_ror:8: with the step before, all four quads of the 16-lane row
      v[e] += __shfl_xor(v[e], 16, 64);
      v[e] += __shfl_xor(v[e], 32, 64);
    }
    __syncthreads();
    if (l < 2) {
#pragma unroll
      for (int e = 0; e < 3; ++e) red[(w * 2 + l) * 4 + e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      T s = 0.f;
#pragma unroll
      for (int i = 0; i < XWV; ++i) s += red[(i * 2 + (cl & 1)) * 4 + e];
      v[e] = s;
    }
  }
  // H as cols_hamiltonian.  The kinetic term of the K = 2 solve needs ONE product: with x2 = z - r1 + c2, z = S g, r1 = S (e . z),
  // c2 = S (e . r1) and S symmetric, g . r1 = z . (e . z) and g . c2 = z . (e . r1), so g . x2 = sum_i [g_i z_i - e_i z_i (z_i - r1_i)].
  __device__ __forceinline__ void hamiltonian(uint32_t n, uint32_t sub, const T (&Xv)[1], const T (&gv)[1], T& H, T& logp, T (&Pd_out)[1],
                                              T (&Sg_out)[1], T& kin_out, T& ld_out) {
    const T X = Xv[0], g = gv[0];
    T evv[1] = {0.f};
    if (a.has_jitter) jitter_one(n, sub, evv);
    const T ev = evv[0], dr = X - mu_r[0];
    EV[own_off] = ev;
    DV[own_off] = dr;
    GV[own_off] = g;
    __syncthreads();
    bf4 Pdv = {0.f, 0.f, 0.f, 0.f}, x0v = {0.f, 0.f, 0.f, 0.f}, s2v = {0.f, 0.f, 0.f, 0.f};
    prod2(Pa, DV, Sa, GV, Pdv, x0v);
    T s2[1] = {0.f}, x0a[1], rv1[1];
    extract(Pdv, Pd_out);
    extract(x0v, x0a);
    const T Pd = Pd_out[0], x0 = x0a[0];
    if (a.has_jitter) { prod1(Sa, EV, true, s2v); extract(s2v, s2); }        // second-order log-det term: (S . S) e
    Sg_out[0] = x0;
    T v[3];
    v[0] = dr * Pd;
    v[2] = a.has_jitter ? ev * (sd_r[0] - 0.5f * s2[0]) : 0.f;               // log|P + E| = log|P| + tr(SE) - 1/2 tr((SE)^2) + ...
    W0[own_off] = ev * x0;
    __syncthreads();
    bf4 rv = {0.f, 0.f, 0.f, 0.f};
    prod1(Sa, W0, false, rv);
    extract(rv, rv1);
    const T r1 = rv1[0];
    v[1] = fmaf(g, x0, -(ev * x0) * (x0 - r1));
    sums(v);
    const float pi_term = (float)a.D * 1.8378770351409912f;  // S:712
    logp = a.log_norm - 0.5f * v[0];
    H = -logp + 0.5f * pi_term + 0.5f * (a.logdetP + v[2]) + 0.5f * v[1];
    kin_out = v[1]; ld_out = v[2];
  }
  // the L steps of one trajectory (S:427-461) and the flush phase
  __device__ __forceinline__ void steps(uint32_t n, T (&Xv)[1], T (&gv)[1], T (&yv)[1], T (&zv)[1]) {
    T &X = Xv[0], &g = gv[0], &y = yv[0], &z = zv[0];
    const T mu = mu_r[0], hc = 0.5f, rc = a.rot_c, rs = a.rot_s;
    T qB = 0.f;                                             // e . r1 of the last B pair: its c2 = S qB is still owed to theta
    for (int lstep = 0; lstep < a.L; ++lstep) {
      const uint32_t k0 = 2u + 8u * (uint32_t)lstep;
      // S:429-433: U moves first and solves with sub-stream k0 + 2, V with k0 + 1; S:454-458: V first (k0 + 7), U second (k0 + 4)
      T eA, eB;
      jitter_pair(n, setV ? k0 + 1u : k0 + 2u, setV ? k0 + 7u : k0 + 4u, eA, eB);
      // ---- A pair  (phi_A/2, phi_B/2  S:429-433)
      g = fmaf(-ehU, y, g);
      z = fmaf(-ehU, X - mu, z);
      const T aA = eA * z;
      WA[own_off] = aA;
      WA[def_off] = qB;
      __syncthreads();
      bf4 r = {0.f, 0.f, 0.f, 0.f};
      prod1(Sa, WA, false, r);
      T r1, c2;
      extract2(r, r1, c2);
      X = fmaf(eh, c2, X);                                  // the previous B pair's second-order term, one phase late
      z = fmaf(zc2, c2, z);
      const T qA = eA * r1;
      X = fmaf(eh, z - r1, X);                              // x1 = z - r1
      y = fmaf(eh, g - (aA - qA), y);                       // P x2 = g - e . x1,  e . x1 = e . z - e . r1
      g = fmaf(-ehV, y, g);                                 // (z of the second mover is evaluated afresh below)
      // ---- phi_C  S:447-450, sequential (Q1), both sets compute it; theta still lacks eh c2 of the A pair
      {
        const T pX = partner(X), pg = partner(g);
        T xx = setV ? pX : X, b = setV ? pg : g, xc = setV ? X : pX, bc = setV ? g : pg;
        xx = hc * ((xx + xc) + rc * (xx - xc) + rs * (b - bc));
        b = hc * ((b + bc) - rs * (xx - xc) + rc * (b - bc));
        xc = hc * ((xx + xc) - rc * (xx - xc) - rs * (b - bc));
        bc = hc * ((b + bc) + rs * (xx - xc) - rc * (b - bc));
        X = setV ? xc : xx; g = setV ? bc : b;
      }
      DV[own_off] = X - mu;
      GV[own_off] = g;
      GV[def_off] = qA;
      __syncthreads();
      bf4 p1 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
      prod2(Pa, DV, Sa, GV, p1, s1);
      extract(p1, yv);
      T c2a;
      extract2(s1, z, c2a);
      // the rotation's image of (eh c2_U, 0, eh c2_V, 0): theta and momentum parts; P c2 = q (no product)
      const T pc2 = partner(c2a), pq = partner(qA);
      X = fmaf(kXo, c2a, fmaf(kXp, pc2, X));
      y = fmaf(kXo, qA, fmaf(kXp, pq, y));
      const T dg = fmaf(kGo, c2a, kGp * pc2);
      g += dg;                                              // z = S g still lacks S dg: next phase
      // ---- B pair  (phi_B/2, phi_A/2  S:454-458)
      g = fmaf(-ehV, y, g);
      z = fmaf(-ehV, X - mu, z);
      const T aB = eB * z;
      WB[own_off] = aB;
      WB[def_off] = dg;
      __syncthreads();
      bf4 r2 = {0.f, 0.f, 0.f, 0.f};
      prod1(Sa, WB, false, r2);
      T r1b, sdg;
      extract2(r2, r1b, sdg);
      z += sdg;
      qB = eB * r1b;
      X = fmaf(eh, z - r1b, X);
      y = fmaf(eh, g - (aB - qB), y);
      g = fmaf(-ehU, y, g);
      z = fmaf(-ehU, X - mu, z);
    }
    // ---- flush: c2 of the last B pair.  (It could ride in the idle columns of the closing Hamiltonian's first product, with
    // P (theta - mu) += eh qB through P S = 1 - measured +3 % - but then the P (theta' - mu) a trajectory hands to the next one
    // is not the product a fresh launch computes from theta': results would depend, in the last bit, on how a run is cut
    // into launches.  tests/test_gpu_rmhmc.py::test_fused_workspace_passes_are_equivalent holds that line.)
    WA[own_off] = 0.f;
    WA[def_off] = qB;
    __syncthreads();
    bf4 r = {0.f, 0.f, 0.f, 0.f};
    prod1(Sa, WA, false, r);
    T r1, c2;
    extract2(r, r1, c2);
    X = fmaf(eh, c2, X);
  }
};

template <bool CO>
__global__ __launch_bounds__(XNT, CO ? 2 : 1) void rmhmc_uvc_kernel(FusedArgs<float> a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  UvcTile t(a, reinterpret_cast<float*>(smem_raw));
  cols_trajectories(a, t);
}

// ---- TWO chains per workgroup (513 ... 1024 chains: two workgroups per CU under the 256-register cap; 257 ... 512 chains: one) ----
// All four columns of the matrix instruction are in use (chain 0's U and V, chain 1's U and V), so there are no idle columns to
// defer into: the schedule is rmhmc_uv_kernel<2>'s (cols_steps: K refinement phases per pair of half steps + one phase after the
// rotation, any K).  What is taken over from the one-chain kernel above is the element-wise layout: the two parities of a row
// block hold the same four rows of a column; here lane (column cl, parity kp) OWNS rows row0 + kp and row0 + 2 + kp - two values
// per lane instead of four duplicated ones, half the element-wise instructions, one 8-byte LDS store per published vector - and
// the branch-free half steps (the set that moves first is selected by a per-lane coefficient, not by divergent control flow).
struct Uvc2Tile : ColsLane {
  static constexpr int NV = 2, NC = 2, NBUF = 9;       // LDS vector matrices: DV GV EV W0 W1 + 4 solve buffers [pair][iteration parity]
  typedef float bf2 __attribute__((ext_vector_type(2)));
  T *WS, *red;                     // half steps: refinement vectors | [XWV][XNC][4]
  int cidx, own_off, row[2];
  bool rok[2], rok_p[2], writer, row_writer;
  T mu_r[2], sd_r[2], ehU, ehV;

  __device__ __forceinline__ Uvc2Tile(const FusedArgs<float>& a_, T* lds) : ColsLane(a_, lds) {
    WS = W0 + 2 * MSZ; red = WS + 4 * MSZ;
    cidx = cl >> 1;
    writer = !setV && w == 0 && (l >> 2) == 0; row_writer = !setV;
    row[0] = row0 + kpar; row[1] = row[0] + 2;            // the two rows this lane owns (column cl)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      rok[i] = row[i] < a.D; rok_p[i] = (row[i] ^ 1) < a.D;
      mu_r[i] = rok[i] ? a.mu[row[i]] : 0.f;
      sd_r[i] = rok[i] ? a.S[(int64_t)row[i] * a.D + row[i]] : 0.f;
    }
    zero_lds(NBUF * MSZ + XWV * XNC * 4);
    ehU = setV ? 0.f : eh; ehV = setV ? eh : 0.f;
    own_off = cl * XLD + kpar * XHL + (row0 >> 1);        // rows row[0], row[1]: two consecutive floats of this parity's half
  }
  __device__ __forceinline__ void put(T* X, const T (&v)[2]) const { *reinterpret_cast<bf2*>(X + own_off) = bf2{v[0], v[1]}; }
  // rows row[0], row[1] of this lane's column: the parity sums
  __device__ __forceinline__ void extract(const bf4& acc, T (&v)[2]) const {
    const T m01 = khi ? acc[1] : acc[0], o01 = khi ? acc[0] : acc[1];
    const T m23 = khi ? acc[3] : acc[2], o23 = khi ? acc[2] : acc[3];
    v[0] = m01 + other_parity(o01);
    v[1] = m23 + other_parity(o23);
  }
  __device__ __forceinline__ T dot(const T (&x)[2], const T (&y)[2]) const { return x[0] * y[0] + x[1] * y[1]; }
  __device__ __forceinline__ void sums(T (&v)[3]) const {
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      v[e] += quad_dpp<0x124>(v[e]);                       // row_ror:4
      v[e] += other_parity(v[e]);
      v[e] += __shfl_xor(v[e], 16, 64);
      v[e] += __shfl_xor(v[e], 32, 64);
    }
    __syncthreads();
    if (l < 4) {
#pragma unroll
      for (int e = 0; e < 3; ++e) red[(w * XNC + l) * 4 + e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      T s = 0.f;
#pragma unroll
      for (int i = 0; i < XWV; ++i) s += red[(i * XNC + cl) * 4 + e];
      v[e] = s;
    }
  }
  __device__ __forceinline__ void jitter_one(uint32_t n, uint32_t sub, T (&e)[2]) const {
    const U4 r = philox_block(a.seed, chain, n, PURPOSE_JITTER, sub, (uint32_t)(row0 >> 2));
    e[0] = (live && rok[0]) ? a.jitter * u23<T>(khi ? r.y : r.x) : 0.f;
    e[1] = (live && rok[1]) ? a.jitter * u23<T>(khi ? r.w : r.z) : 0.f;
  }
  // both jitter vectors of a step for this column: the even parity draws the A pair's block, the odd parity the B pair's, each
  // hands the other the elements of the other's rows
  __device__ __forceinline__ void jitter_pair(uint32_t n, uint32_t subA, uint32_t subB, T (&eA)[2], T (&eB)[2]) const {
    const U4 r = philox_block(a.seed, chain, n, PURPOSE_JITTER, khi ? subB : subA, (uint32_t)(row0 >> 2));
    const T ma = (live && rok[0]) ? a.jitter * u23<T>(khi ? r.y : r.x) : 0.f;
    const T mb = (live && rok[1]) ? a.jitter * u23<T>(khi ? r.w : r.z) : 0.f;
    const T oa = other_parity((live && rok_p[0]) ? a.jitter * u23<T>(khi ? r.x : r.y) : 0.f);
    const T ob = other_parity((live && rok_p[1]) ? a.jitter * u23<T>(khi ? r.z : r.w) : 0.f);
    eA[0] = khi ? oa : ma; eA[1] = khi ? ob : mb;
    eB[0] = khi ? ma : oa; eB[1] = khi ? mb : ob;
  }
  // every lane runs both kicks of a pair; the coefficient of the set that does not move at this point is zero
  __device__ __forceinline__ void kick(bool second, bool after, const T (&X)[2], T (&g)[2], const T (&y)[2], T (&z)[2]) const {
    const T c = second != after ? ehV : ehU;
    g[0] = fmaf(-c, y[0], g[0]); g[1] = fmaf(-c, y[1], g[1]);
    z[0] = fmaf(-c, X[0] - mu_r[0], z[0]); z[1] = fmaf(-c, X[1] - mu_r[1], z[1]);
  }
  __device__ __forceinline__ void steps(uint32_t n, T (&X)[2], T (&g)[2], T (&y)[2], T (&z)[2]) { cols_steps(*this, n, X, g, y, z); }
  __device__ __forceinline__ void hamiltonian(uint32_t n, uint32_t sub, const T (&X)[2], const T (&g)[2], T& H, T& logp, T (&Pd)[2],
                                              T (&Sg)[2], T& kin, T& ld) {
    cols_hamiltonian(*this, n, sub, X, g, H, logp, Pd, Sg, kin, ld);
  }
};

template <bool CO>
__global__ __launch_bounds__(XNT, CO ? 2 : 1) void rmhmc_uvc2_kernel(FusedArgs<float> a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  Uvc2Tile t(a, reinterpret_cast<float*>(smem_raw));
  cols_trajectories(a, t);
}

int g_rmhmc_uvc = 1;         // tuning key "rmhmc_uvc" (default 1): one-chain groups with K == 2 and jitter run on rmhmc_uvc_kernel, two-chain groups on rmhmc_uvc2_kernel; 0 = rmhmc_uv_kernel

int rmhmc_uvc2_launch(const FusedArgs<float>& a, bool co, hipStream_t s) {
  const size_t bytes = (size_t)(Uvc2Tile::NBUF * XNC * XLD + XWV * XNC * 4) * sizeof(float);
  const int64_t ngroup = (a.C + 1) / 2;
  const int grid = (int)(ngroup < 8192 ? ngroup : 8192);
  note_route("rmhmc_uvc2_kernel<%s>", co ? "co" : "solo");
  if (co) rmhmc_uvc2_kernel<true><<<grid, XNT, bytes, s>>>(a);
  else rmhmc_uvc2_kernel<false><<<grid, XNT, bytes, s>>>(a);
  return HTA_OK;
}

int rmhmc_uvc_launch(const FusedArgs<float>& a, bool co, hipStream_t s) {
  const size_t bytes = (size_t)(UvcTile::NBUF * XNC * XLD + XWV * 2 * 4) * sizeof(float);
  const int grid = (int)(a.C < 8192 ? a.C : 8192);
  note_route("rmhmc_uvc_kernel<%s>", co ? "co" : "solo");
  if (co) rmhmc_uvc_kernel<true><<<grid, XNT, bytes, s>>>(a);
  else rmhmc_uvc_kernel<false><<<grid, XNT, bytes, s>>>(a);
  return HTA_OK;
}

}  // namespace hta
