// The trajectory shell of the explicit-RMHMC kernels whose chains are COLUMNS of the 16-block instruction
// v_mfma_f32_4x4x1_16b_f32 (rmhmc_uv.hip: rmhmc_uv_kernel, four duplicated values per lane; rmhmc_uvc.hip: rmhmc_uvc2_kernel, two
// values per lane, and rmhmc_uvc_kernel, one).  A chain fills two columns: its state set U = (theta, p) and the copy
// V = (theta_c, p_c) of S:425-426, in the lanes l and l ^ 1 of a quad.  Same Philox streams, same update order and bookkeeping
// (Q1, Q2, Q4) as the one-chain rmhmc_fused_kernel, which is the parity reference of all three.
//
// Written once here: the lane geometry, the operand load and the products (ColsLane), the chain-group / trajectory loop with the
// momentum prefetch, the hand-over of a trajectory's closing Hamiltonian to the next one, the Metropolis test and every store
// (cols_trajectories), and the step of the kernels that run the schedule of rows4_trajectories (rmhmc_rows4_dev.hpp: K
// refinement phases per pair of half steps + one refresh phase after the rotation, any K): cols_steps, cols_solve,
// cols_hamiltonian.  A per-kernel Tile (derived from ColsLane) holds what really differs:
//   NV, NC                        values per lane (4, 2, 1); chains per workgroup
//   cidx, row[NV], rok[NV]        the chain column of this lane and the rows it owns (rok: row < D)
//   mu_r[NV], sd_r[NV]            mu and diag(S) at those rows
//   writer, row_writer            the one lane per chain that writes H_old / H_new / accept / reject_count; the lanes that
//                                 write their rows of the samples and of the final state (set U, one of any duplicates)
//   WS, ...                       the LDS vector matrices beyond DV GV EV W0 W1 (ColsLane)
//   put(X, v)                     this lane's values into vector matrix X
//   extract(acc, v)               accumulator -> owned values (with the sum over the two contraction parities)
//   dot(x, y), sums(v)            the sum over this lane's rows, in the kernel's own order; three sums per set over all rows,
//                                 complete in every lane of the set
//   jitter_one(n, sub, e), jitter_pair(n, subA, subB, eA, eB)     the jitter of a Hamiltonian; of the two solves of a step
//   kick(second, after, X, g, y, z)   (cols_steps only) g -= eh y, z -= eh (X - mu) in the set whose momentum moves at this point
//   hamiltonian(...), steps(...)  cols_hamiltonian / cols_steps, or the kernel's own (rmhmc_uvc_kernel: deferred second-order
//                                 products, one flush phase per trajectory)
// Rules the shared code keeps: a cross-lane DPP read stands outside any branch that is not uniform over the quad (inside an arm
// it would run under that arm's lane mask); the momentum loads are unconditional, with masks the optimiser cannot see through;
// -ffp-contract=on contracts within a statement only: splitting or joining an arithmetic statement changes the bits.
#pragma once
#include "rmhmc_fused_dev.hpp"

namespace hta {

template <int CTRL> __device__ __forceinline__ float quad_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float partner(float v) { return quad_dpp<0xB1>(v); }    // the other set's value of the same row: quad_perm [1,0,3,2]
__device__ __forceinline__ float of_set_u(float v) { return quad_dpp<0xA0>(v); }   // the U column's value of this chain: [0,0,2,2]
__device__ __forceinline__ float of_set_v(float v) { return quad_dpp<0xF5>(v); }   // the V column's: [1,1,3,3]

// Rows x contraction parity inside a wave, operand fetch through the B-broadcast modifier, LDS layout: rmhmc_fused_dev.hpp.
// lane bits: [1:0] column = 2 chain + set, [2] low bit of the row block, [3] contraction parity, [5:4] 16-lane group
struct ColsLane {
  typedef float T;
  static constexpr int MSZ = XNC * XLD;
  const FusedArgs<float>& a;
  T *DV, *GV, *EV, *W0;            // X - mu (operand of P: refresh phase, Hamiltonians) | momenta (operand of S there) |
                                   // Hamiltonian: the jitter | Hamiltonian: refinement vectors W0, W1
  int tid, w, l, cl, grp, kpar, row0, b_off;
  bool khi, setV, live;
  uint64_t chain;
  T eh, Sa[XKJ], Pa[XKJ];          // this lane's share of S and P: registers for the whole launch

  __device__ __forceinline__ ColsLane(const FusedArgs<float>& a_, T* lds) : a(a_) {
    DV = lds; GV = DV + MSZ; EV = GV + MSZ; W0 = EV + MSZ;
    tid = threadIdx.x; w = tid >> 6; l = tid & 63; cl = l & 3; grp = l >> 4;
    kpar = (l >> 3) & 1; khi = kpar != 0; setV = (cl & 1) != 0;
    const int D = a.D, rb = 2 * grp + ((l >> 2) & 1);
    row0 = 32 * w + 4 * rb;                               // the row block's four rows; this lane SUPPLIES matrix row arow
    const int arow = row0 + cl;
#pragma unroll
    for (int j = 0; j < XKJ; ++j) {
      const int k = 2 * j + kpar;
      const bool ok = arow < D && k < D;
      Sa[j] = ok ? a.S[(int64_t)k * D + arow] : 0.f;      // symmetric: column arow, coalesced over the lanes
      Pa[j] = ok ? a.P[(int64_t)k * D + arow] : 0.f;
    }
    eh = 0.5f * a.eps;
    b_off = cl * XLD + kpar * XHL + 4 * grp;              // this group's chunk of a super-chunk of four
    chain = 0; live = false;
  }
  __device__ __forceinline__ void zero_lds(int n) const { for (int e = tid; e < n; e += XNT) DV[e] = 0.f; }

  __device__ __forceinline__ void fetch(const T* X, bf4 (&c)[XSQ]) const {
#pragma unroll
    for (int Q = 0; Q < XSQ; ++Q) c[Q] = *reinterpret_cast<const bf4*>(X + b_off + 16 * Q);
  }
  // acc1 += A1 X1, acc2 += A2 X2 for all four columns (one accumulator chain each: two chains per product would need s_nops,
  // the two products interleave); this lane's contraction parity only
  __device__ __forceinline__ void prod2(const T (&A1)[XKJ], const T* X1, const T (&A2)[XKJ], const T* X2, bf4& acc1, bf4& acc2) const {
    bf4 c1[XSQ], c2[XSQ];
    fetch(X1, c1);
    fetch(X2, c2);
    __builtin_amdgcn_sched_barrier(0);
    static_for(std::make_integer_sequence<int, XQ>{}, [&](auto qc) {
      constexpr int q = decltype(qc)::value;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc1 = mfma_from_group<q % 4>(A1[4 * q + u], c1[q / 4][u], acc1);
        acc2 = mfma_from_group<q % 4>(A2[4 * q + u], c2[q / 4][u], acc2);
      }
    });
  }
  // one product on two accumulator chains (k in the order 0 2 | 1 3 of every chunk); squared: (A . A) X
  __device__ __forceinline__ void prod1(const T (&A1)[XKJ], const T* X1, bool squared, bf4& acc) const {
    bf4 c1[XSQ], sb = {0.f, 0.f, 0.f, 0.f};
    fetch(X1, c1);
    __builtin_amdgcn_sched_barrier(0);
    static_for(std::make_integer_sequence<int, XQ>{}, [&](auto qc) {
      constexpr int q = decltype(qc)::value;
#pragma unroll
      for (int u = 0; u < 4; u += 2) {
        const T a0 = A1[4 * q + u], a1 = A1[4 * q + u + 1];
        acc = mfma_from_group<q % 4>(squared ? a0 * a0 : a0, c1[q / 4][u], acc);
        sb = mfma_from_group<q % 4>(squared ? a1 * a1 : a1, c1[q / 4][u + 1], sb);
      }
    });
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += sb[e];
  }
};

// x = (P + diag(e))^-1 g from x0 = S g: K phases (one barrier, one product each); wv returns e . x_(K-1) (zero without jitter).
// WB: two vector matrices, written before the barrier of a phase and read in that phase only.
template <class Tile>
__device__ __forceinline__ void cols_solve(Tile& t, float* WB, const float (&e)[Tile::NV], const float (&x0)[Tile::NV],
                                           float (&x)[Tile::NV], float (&wv)[Tile::NV]) {
  constexpr int NV = Tile::NV;
#pragma unroll
  for (int i = 0; i < NV; ++i) { x[i] = x0[i]; wv[i] = 0.f; }
  for (int it = 0; it < t.a.K; ++it) {
    float* A = WB + (it & 1) * Tile::MSZ;
#pragma unroll
    for (int i = 0; i < NV; ++i) wv[i] = e[i] * x[i];
    t.put(A, wv);
    __syncthreads();
    bf4 r = {0.f, 0.f, 0.f, 0.f};
    t.prod1(t.Sa, A, false, r);
    float rv[NV];
    t.extract(r, rv);
#pragma unroll
    for (int i = 0; i < NV; ++i) x[i] = x0[i] - rv[i];
  }
}

// H = -log p + D/2 log 2 pi + 1/2 log|G| + 1/2 g^T G^-1 g  (S:731) of this column's (X, g); also returns P (X - mu) and S g
// (n, sub: per lane - in the Hamiltonian at a trajectory's end the V column evaluates the NEXT trajectory's momentum terms)
template <class Tile>
__device__ __forceinline__ void cols_hamiltonian(Tile& t, uint32_t n, uint32_t sub, const float (&X)[Tile::NV], const float (&g)[Tile::NV],
                                                 float& H, float& logp, float (&Pd_out)[Tile::NV], float (&Sg_out)[Tile::NV],
                                                 float& kin_out, float& ld_out) {
  typedef float T;
  constexpr int NV = Tile::NV;
  const FusedArgs<float>& a = t.a;
  T ev[NV], dr[NV], x0[NV], s2[NV], ldt[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) { ev[i] = 0.f; s2[i] = 0.f; }
  if (a.has_jitter) t.jitter_one(n, sub, ev);
#pragma unroll
  for (int i = 0; i < NV; ++i) dr[i] = X[i] - t.mu_r[i];
  t.put(t.EV, ev);
  t.put(t.DV, dr);
  t.put(t.GV, g);
  __syncthreads();
  bf4 Pdv = {0.f, 0.f, 0.f, 0.f}, x0v = {0.f, 0.f, 0.f, 0.f}, s2v = {0.f, 0.f, 0.f, 0.f};
  t.prod2(t.Pa, t.DV, t.Sa, t.GV, Pdv, x0v);
  t.extract(Pdv, Pd_out);
  t.extract(x0v, x0);
  if (a.has_jitter) { t.prod1(t.Sa, t.EV, true, s2v); t.extract(s2v, s2); }     // second-order log-det term: (S . S) e
#pragma unroll
  for (int i = 0; i < NV; ++i) { Sg_out[i] = x0[i]; ldt[i] = t.sd_r[i] - 0.5f * s2[i]; }
  T v[3];
  v[0] = t.dot(dr, Pd_out);
  v[2] = a.has_jitter ? t.dot(ev, ldt) : 0.f;             // log|P + E| = log|P| + tr(SE) - 1/2 tr((SE)^2) + ...
  T xr[NV], wv[NV];
  cols_solve(t, t.W0, ev, x0, xr, wv);
  v[1] = t.dot(g, xr);
  t.sums(v);
  const float pi_term = (float)a.D * 1.8378770351409912f;   // S:712
  logp = a.log_norm - 0.5f * v[0];
  H = -logp + 0.5f * pi_term + 0.5f * (a.logdetP + v[2]) + 0.5f * v[1];
  kin_out = v[1]; ld_out = v[2];
}

// The L steps of one trajectory (S:427-461) on the tracked schedule derived in rows4_trajectories: per chain exactly two vectors
// are in flight in every product phase, one of U = (theta, p, y = P (theta - mu), z = S p) and one of V - the chain's two
// columns - so a phase is ONE product for both solves of every chain, and the element-wise work of a pair of half steps splits
// over the two columns:
//   first  (the set whose momentum moves first: U in S:429-433, V in S:454-458):  kick;  solve;  X += eh x;  y += eh (g - w)
//   second:                                                                         solve;  X += eh x;  y += eh (g - w);  kick
// with kick: g -= eh y, z -= eh (X - mu); x = (P + E)^-1 g from x_0 = z and w = e . x_(K-1).  The rotation phi_C (S:447-450) needs
// both sets in one lane: the columns exchange their X and g through a DPP quad permutation, both compute the (sequential, Q1)
// rotation and keep their half; right after it y and z are evaluated afresh (P (X - mu) and S g: one phase).
// Per step at K = 2: 5 phases, 312 matrix instructions per wave.  t.WS: refinement vectors [pair of the step][iteration parity].
template <class Tile>
__device__ __forceinline__ void cols_steps(Tile& t, uint32_t n, float (&X)[Tile::NV], float (&g)[Tile::NV], float (&y)[Tile::NV],
                                           float (&z)[Tile::NV]) {
  typedef float T;
  constexpr int NV = Tile::NV;
  const FusedArgs<float>& a = t.a;
  const T eh = t.eh;
  const bool setV = t.setV;
  // one pair of half steps for this column (second: the pair S:454-458, in which V moves first); WB: its two refinement matrices
  auto half_pair = [&](bool second, const T (&e)[NV], T* WB) {
    t.kick(second, false, X, g, y, z);
    T x[NV], wv[NV];
    cols_solve(t, WB, e, z, x, wv);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      X[i] = fmaf(eh, x[i], X[i]);
      y[i] = fmaf(eh, g[i] - wv[i], y[i]);                  // P x = g - e . x_(K-1)
    }
    t.kick(second, true, X, g, y, z);
  };
  for (int lstep = 0; lstep < a.L; ++lstep) {
    const uint32_t k0 = 2u + 8u * (uint32_t)lstep;
    // jitter: in S:429-433 the set that moves first (U) solves with sub-stream k0 + 2 and V with k0 + 1; in S:454-458 V moves
    // first (k0 + 7) and U second (k0 + 4)
    T eA[NV], eB[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) { eA[i] = 0.f; eB[i] = 0.f; }
    if (a.has_jitter) t.jitter_pair(n, setV ? k0 + 1u : k0 + 2u, setV ? k0 + 7u : k0 + 4u, eA, eB);
    half_pair(false, eA, t.WS);                             // phi_A/2, phi_B/2  S:429-433
    if (a.K == 0) __syncthreads();                          // (no solve phase since the last reads of DV / GV)
    T dv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {                          // phi_C  S:447-450, sequential (Q1), both columns compute it
      const T pX = partner(X[i]), pg = partner(g[i]);
      T xx = setV ? pX : X[i], b = setV ? pg : g[i], xc = setV ? X[i] : pX, bc = setV ? g[i] : pg;
      const T h = 0.5f, cc = a.rot_c, ss = a.rot_s;
      xx = h * ((xx + xc) + cc * (xx - xc) + ss * (b - bc));
      b = h * ((b + bc) - ss * (xx - xc) + cc * (b - bc));
      xc = h * ((xx + xc) - cc * (xx - xc) - ss * (b - bc));
      bc = h * ((b + bc) + ss * (xx - xc) - cc * (b - bc));
      X[i] = setV ? xc : xx; g[i] = setV ? bc : b;
      dv[i] = X[i] - t.mu_r[i];
    }
    t.put(t.DV, dv);                                        // the tracked products of the rotated state, afresh
    t.put(t.GV, g);
    __syncthreads();
    bf4 p1 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    t.prod2(t.Pa, t.DV, t.Sa, t.GV, p1, s1);
    t.extract(p1, y);
    t.extract(s1, z);
    half_pair(true, eB, t.WS + 2 * Tile::MSZ);              // phi_B/2, phi_A/2  S:454-458
  }
  if (a.K == 0) __syncthreads();
}

template <class Tile>
__device__ __forceinline__ void cols_trajectories(const FusedArgs<float>& a, Tile& t) {
  typedef float T;
  constexpr int NV = Tile::NV;
  const int D = a.D;
  const bool setV = t.setV;
  const int64_t ngroup = (a.C + Tile::NC - 1) / Tile::NC;
  for (int64_t cg = blockIdx.x; cg < ngroup; cg += gridDim.x) {
    const int64_t c = Tile::NC * cg + t.cidx;
    const bool live = t.cidx < Tile::NC && (Tile::NC == 1 || c < a.C);   // (a one-chain group is never partial)
    t.live = live;
    t.chain = a.chain_offset + (uint64_t)(live ? c : 0);
    T scur[NV], X[NV], g[NV], y[NV], z[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) scur[i] = (live && t.rok[i]) ? a.cur[c * D + t.row[i]] : 0.f;
    const int64_t cs = live ? c : 0;                        // (a dead column reads chain 0's rows and discards them)
    int rmask[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) { rmask[i] = -(int)t.rok[i]; asm volatile("" : "+v"(rmask[i])); }
    // this lane's rows of the pre-drawn momentum of local trajectory tt: UNCONDITIONAL loads (a lane without a row reads
    // element 0 of the chain's row and discards it), so that they issue back to back and are waited for once
    // (offsets masked arithmetically with masks the optimiser cannot see through: a select on the index - or a mask it can
    //  trace back to rok - comes back as a branch around each load, with a wait inside)
    auto momentum_raw = [&](int tt, T (&v)[NV]) {
      const T* prow = a.p_ws + ((int64_t)tt * a.C + cs) * D;
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] = prow[t.row[i] & rmask[i]];
    };
    auto momentum_use = [&](T (&v)[NV], T (&out)[NV]) {       // (the empty asm pins the first use of the loaded registers HERE)
#pragma unroll
      for (int i = 0; i < NV; ++i) { asm volatile("" : "+v"(v[i])); out[i] = (live && t.rok[i]) ? v[i] : 0.f; }
    };
    int32_t rejected = 0;
    __syncthreads();                                        // the previous group's last reads of the vector matrices
    // H_old of trajectory t + 1 needs, besides -log p of the current point, only terms of the NEW momentum and jitter
    // (1/2 p^T G^-1 p and log |G|: the curvature is constant) - none of them waits for trajectory t's outcome.  So the
    // Hamiltonian at the END of trajectory t evaluates them on the side: the V column, idle there, takes p(t+1) and the jitter
    // of (t+1, sub-stream 1) through the same phases, and trajectory t + 1 starts without a Hamiltonian of its own
    // (log p, y = P (theta - mu) of the accepted / kept point are known; z = S p(t+1) comes out of the V column).  The same
    // products in the same order as the separate evaluation: bit-identical results, four phases less per trajectory.  Not
    // taken for a launch's first trajectory and after the Q2 reset to params_init (its log p is not known).
    bool have_next = false;
    T gn[NV], y_next[NV], z_next[NV], H0_next = 0.f, lp_next = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) { gn[i] = 0.f; y_next[i] = 0.f; z_next[i] = 0.f; }
    for (int tr = 0; tr < a.n_traj; ++tr) {
      const uint32_t n = (uint32_t)(a.traj_offset + tr);
      // ---- gibbs: p = chol(G(theta)) z, drawn ahead by the momentum kernel (S:183-184); theta_c = theta, p_c = p (S:425-426)
      T H0, H1, lp0, lp1, kin, ld;
      if (have_next) {
#pragma unroll
        for (int i = 0; i < NV; ++i) { g[i] = gn[i]; X[i] = scur[i]; y[i] = y_next[i]; z[i] = z_next[i]; }
        H0 = H0_next; lp0 = lp_next;
      } else {
        T raw[NV];
        momentum_raw(tr, raw);
        momentum_use(raw, g);
#pragma unroll
        for (int i = 0; i < NV; ++i) X[i] = scur[i];
        t.hamiltonian(n, 1, X, g, H0, lp0, y, z, kin, ld);  // S:971 -> S:822
      }
      // the NEXT trajectory's momentum rows are requested here, a whole trajectory before their first use (the V column of this
      // trajectory's last Hamiltonian): requested there, each load was followed by its own s_waitcnt vmcnt(0) - exposed memory
      // round trips of a wave that has nothing else to issue
      const bool pre = tr + 1 < a.n_traj;
      T gn_raw[NV], y_start[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) { gn_raw[i] = 0.f; y_start[i] = y[i]; }
      if (pre) momentum_raw(tr + 1, gn_raw);
      t.steps(n, X, g, y, z);                               // S:427-461
      // ---- H_new on the un-augmented pair = set U (S:989, Q4); in the V column: the next trajectory's momentum terms
      T Pd1[NV], Sg1[NV], Xh[NV], gh[NV];
      if (pre) momentum_use(gn_raw, gn);
      const bool nextcol = setV && pre;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        Xh[i] = of_set_u(X[i]);                             // both columns at the proposal theta': the V column's P (theta' - mu) is not used
        const T gu = of_set_u(g[i]);
        gh[i] = nextcol ? gn[i] : gu;
      }
      t.hamiltonian(nextcol ? n + 1u : n, nextcol ? 1u : 2u + 8u * (uint32_t)a.L, Xh, gh, H1, lp1, Pd1, Sg1, kin, ld);
      // ---- Metropolis test + bookkeeping (S:1000-1026, S:1045-1057) on the U column's values, mirrored in the V column
      const T H0u = of_set_u(H0), H1u = of_set_u(H1), lp1u = of_set_u(lp1);
      const T u = u23<T>(philox_block(a.seed, t.chain, n, PURPOSE_MH, 0, 0).x);
      const bool acc = mh_accept<T>(H0u, H1u, lp1u, u);
      const bool reset = (!acc) && ((int)n == a.burn + 1);  // Q2
      // The columns of a group decide TOGETHER whether the next trajectory starts from the hand-over.  The Hamiltonian a chain runs
      // for itself after its reset holds barriers, LDS exchanges and matrix instructions, and those take their operand rows from all
      // four columns of a quad - the other chain's and the idle ones too: under one chain's lane mask whatever is computed or
      // reloaded for an operand inside that branch stays stale in the masked lanes (seen as H_old = -1e8 ... -1e33 after the reset
      // of one chain of a two-chain group in the 256-register instance of rmhmc_uvc2_kernel, and as an H_old off by 6e-3 in
      // rmhmc_uv_kernel<2,co>: tests/test_gpu_rmhmc_traj.py).  Every quad holds every column; a dead or idle column has no say.
      float reset_any = (live && reset) ? 1.f : 0.f;
      reset_any = fmaxf(reset_any, quad_dpp<0xB1>(reset_any));      // quad_perm [1,0,3,2]
      reset_any = fmaxf(reset_any, quad_dpp<0x4E>(reset_any));      // quad_perm [2,3,0,1]
      have_next = pre && reset_any == 0.f;
      {                                                     // H_old, y, z of trajectory t + 1 (the expression of hamiltonian(), same order)
        const T lp0u = of_set_u(lp0), ldv = of_set_v(ld), kinv = of_set_v(kin);
        T Pd1u[NV], Sg1v[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) { Pd1u[i] = of_set_u(Pd1[i]); Sg1v[i] = of_set_v(Sg1[i]); }
        if (have_next) {
          const float pi_term = (float)D * 1.8378770351409912f;
          lp_next = acc ? lp1u : lp0u;
          H0_next = -lp_next + 0.5f * pi_term + 0.5f * (a.logdetP + ldv) + 0.5f * kinv;
#pragma unroll
          for (int i = 0; i < NV; ++i) {
            y_next[i] = acc ? Pd1u[i] : y_start[i];         // (both sets start a trajectory with the same y)
            z_next[i] = Sg1v[i];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        if (live && t.rok[i]) {
          // (the reset value is loaded under a branch of its own: as an arm of the select below it meets the load of scur[i] in
          //  a phi, which the optimiser turns into ONE load through a selected address - scur then lives in scratch)
          T init = 0.f;
          if (reset) init = a.theta_init[c * D + t.row[i]];
          const T vnew = acc ? Xh[i] : (reset ? init : scur[i]);
          scur[i] = vnew;
          if (t.row_writer && a.samples && (int)n > a.burn) a.samples[((int64_t)((int)n - a.burn) * a.C + c) * D + t.row[i]] = vnew;
        }
      }
      if (live && t.writer) {
        if (a.H_old) a.H_old[(int64_t)tr * a.C + c] = H0u;
        if (a.H_new) a.H_new[(int64_t)tr * a.C + c] = H1u;
        if (a.accept) a.accept[(int64_t)tr * a.C + c] = acc ? 1 : 0;
      }
      if (!acc) ++rejected;
    }
    if (live && t.row_writer) {
#pragma unroll
      for (int i = 0; i < NV; ++i) if (t.rok[i]) a.cur[c * D + t.row[i]] = scur[i];
    }
    if (live && t.writer) a.reject_count[c] += rejected;
  }
}

}  // namespace hta
