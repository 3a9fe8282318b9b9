// The trajectory body of the explicit-RMHMC kernels whose lanes own FOUR consecutive rows of one chain's vectors - one Philox
// block of jitter per evaluation - and whose products run on the matrix cores (rmhmc_fused_tiles_dev.hpp: rmhmc_batch_kernel, sixteen
// chains per workgroup; rmhmc_mfma4_kernel, four; launched by rmhmc_fused.hip).  Same streams, same update order and barriers per pass
// as the one-chain rmhmc_fused_kernel (rmhmc_fused_chain_dev.hpp), which is the parity reference of both.
//
// The algorithm is written once here, over a per-kernel Tile that holds what really differs between the kernels:
//   NC, MSZ                       chains per workgroup; floats per LDS vector matrix
//   row0, cl, rok[4], writer      this lane's rows row0 .. row0+3 (rok: row < D) of chain column cl; the one lane per chain that
//                                 writes H_old / H_new / accept / reject_count
//   mu_r[4], sd_r[4]              mu and diag(S) at those rows
//   Sa[], Pa[]                    this lane's share of the matrix operands S and P (registers for the whole launch)
//   PM PMC D0 D1 DC W0 W1 EV      LDS vector matrices; WSA, WSB: the 2 solves x 2 refinement vectors of a step's first / second pair
//   put4(X, v)                    this lane's four values into vector matrix X
//   prod2(A1, X1, A2, X2, c1, c2) c1 += A1 X1, c2 += A2 X2 with one pass over k (A1, A2: Sa or Pa)
//   prod1(X, c), prod1_sq(X, c)   c = S X (the refinement product) and c = (S . S) X (the log-det term), in the kernel's own
//                                 summation order
//   prod4(X1, X2, X3, X4, ...)    P X1, P X2, S X3, S X4
//   block_sums(v)                 three sums per chain over the rows, complete in every lane of the chain's column
#pragma once
#include "rmhmc_fused_dev.hpp"

namespace hta {

template <bool TRACK, class Tile>
__device__ __forceinline__ void rows4_trajectories(const FusedArgs<float>& a, Tile& t) {
  typedef float T;
  constexpr int MSZ = Tile::MSZ;
  const int D = a.D;
  const T eh = 0.5f * a.eps;
  int dpar = 0;
  T ev_r[4] = {0.f, 0.f, 0.f, 0.f};
  uint64_t chain = 0;
  bool live = false;

  auto jitter4 = [&](uint32_t n, uint32_t sub) {            // this lane's four rows are one Philox block (uniform_elem layout)
    if (!a.has_jitter) return;
    const U4 r = philox_block(a.seed, chain, n, PURPOSE_JITTER, sub, (uint32_t)(t.row0 >> 2));
    const T u[4] = {u23<T>(r.x), u23<T>(r.y), u23<T>(r.z), u23<T>(r.w)};
#pragma unroll
    for (int e = 0; e < 4; ++e) ev_r[e] = (live && t.rok[e]) ? a.jitter * u[e] : 0.f;
  };
  // x = (P + diag(e))^-1 m continued from x0 = S m (rmhmc_fused_kernel: refine)
  auto refine = [&](const T (&x0)[4], T (&xr)[4]) {
    for (int it = 0; it < a.K; ++it) {
      const T* wr = (it & 1) ? t.W1 : t.W0;
      T* ww = (it & 1) ? t.W0 : t.W1;
      __syncthreads();
      bf4 sx;
      t.prod1(wr, sx);
      T wv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) { xr[e] = x0[e] - sx[e]; wv[e] = ev_r[e] * xr[e]; }
      t.put4(ww, wv);
    }
  };
  // one half step: upd_x += eh G(X)^-1 m ; upd_g -= eh P (X - mu)   (rmhmc_fused_kernel: half_step)
  auto half_step = [&](uint32_t n, uint32_t sub, const T (&X)[4], const T* m, T (&upd_x)[4], T (&upd_g)[4], T* upd_g_lds) {
    T* d = dpar ? t.D1 : t.D0;
    dpar ^= 1;
    T dv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) dv[e] = t.rok[e] ? X[e] - t.mu_r[e] : 0.f;
    t.put4(d, dv);
    __syncthreads();
    bf4 Pd = {0.f, 0.f, 0.f, 0.f}, x0v = {0.f, 0.f, 0.f, 0.f};
    t.prod2(t.Pa, d, t.Sa, m, Pd, x0v);
    jitter4(n, sub);            // first needed after the products: its Philox rounds issue under the MFMAs
    T x0[4], xr[4], wv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      upd_g[e] -= eh * Pd[e];
      x0[e] = x0v[e]; xr[e] = x0v[e];
      wv[e] = ev_r[e] * x0v[e];
    }
    t.put4(upd_g_lds, upd_g);
    t.put4(t.W0, wv);
    refine(x0, xr);
#pragma unroll
    for (int e = 0; e < 4; ++e) upd_x[e] += eh * xr[e];
  };
  // ---- TRACK: the half steps without their P d and S m products ------------------------------------------------------
  // S = P^-1 is what makes this path possible in the first place, and it also makes two of a half step's K + 2 products
  // redundant.  Keep y = P (theta - mu), y_c = P (theta_c - mu), z = S p, z_c = S p_c next to the four state vectors:
  //   p -= eh P (theta - mu) = eh y           =>  z -= eh (theta - mu)                          (S P = I)
  //   theta_c += eh x,  x = (P + E)^-1 p_c    =>  y_c += eh P x = eh (p_c - e . x_(K-1))         (x_K = S p_c - S (e . x_(K-1)))
  // element-wise, exact for the iteration as implemented.  The solve starts from x_0 = S p_c = z_c: only its K refinement
  // products remain, and the second half step of a pair (position theta_c, momentum the p just updated) no longer depends on
  // the first one's solve: the two solves run side by side, one accumulator chain each - K product phases per PAIR of half
  // steps instead of 2 (K + 1).  The rotation phi_C mixes all four vectors; right after it the four tracked products are
  // evaluated afresh in one phase (so a tracked vector carries at most four element-wise updates of rounding).  Per step at
  // K = 2: 5 barrier-separated phases and 12 products instead of 8 and 16.
  T y[4], yc[4], z[4], zc[4];
  // two independent solves x = (P + E)^-1 m from x_0 = S m, K phases; wa / wb return e . x_(K-1) (zero without jitter)
  auto solve2 = [&](T* WB, const T (&ea)[4], const T (&eb)[4], const T (&x0a)[4], const T (&x0b)[4], T (&xa)[4], T (&xb)[4],
                    T (&wa)[4], T (&wb)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { xa[e] = x0a[e]; xb[e] = x0b[e]; wa[e] = 0.f; wb[e] = 0.f; }
    for (int it = 0; it < a.K; ++it) {
      T* A = WB + (it & 1) * MSZ;                           // read in this phase only; rewritten two phases later
      T* B = A + 2 * MSZ;
#pragma unroll
      for (int e = 0; e < 4; ++e) { wa[e] = ea[e] * xa[e]; wb[e] = eb[e] * xb[e]; }
      t.put4(A, wa);
      t.put4(B, wb);
      __syncthreads();
      bf4 ra = {0.f, 0.f, 0.f, 0.f}, rb = {0.f, 0.f, 0.f, 0.f};
      t.prod2(t.Sa, A, t.Sa, B, ra, rb);
#pragma unroll
      for (int e = 0; e < 4; ++e) { xa[e] = x0a[e] - ra[e]; xb[e] = x0b[e] - rb[e]; }
    }
  };
  // a pair of half steps (S:429-433 and, with the roles of the copies swapped, S:454-458):
  //   a:  g1 -= eh P (X1 - mu)   X2 += eh (P + E_a)^-1 g2        b:  g2 -= eh P (X2 - mu)   X1 += eh (P + E_b)^-1 g1
  // with y1 = P (X1 - mu), y2 = P (X2 - mu), z1 = S g1, z2 = S g2 kept current
  auto pair_tracked = [&](T* WB, uint32_t n, uint32_t suba, uint32_t subb, T (&X1)[4], T (&X2)[4], T (&g1)[4], T (&g2)[4],
                          T (&y1)[4], T (&y2)[4], T (&z1)[4], T (&z2)[4]) {
    T ea[4], eb[4];
    jitter4(n, suba);
#pragma unroll
    for (int e = 0; e < 4; ++e) ea[e] = ev_r[e];
    jitter4(n, subb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      eb[e] = ev_r[e];
      g1[e] -= eh * y1[e];                                  // a's momentum update ...
      z1[e] -= eh * (t.rok[e] ? X1[e] - t.mu_r[e] : 0.f);   // ... and S g1 with it
    }
    T xa[4], xb[4], wa[4], wb[4];
    solve2(WB, ea, eb, z2, z1, xa, xb, wa, wb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      X2[e] += eh * xa[e];                                  // a's position update; P x_a = g2 - e_a . x_a(K-1)
      y2[e] += eh * (g2[e] - wa[e]);
      g2[e] -= eh * y2[e];                                  // b's momentum update
      z2[e] -= eh * (t.rok[e] ? X2[e] - t.mu_r[e] : 0.f);
      X1[e] += eh * xb[e];                                  // b's position update
      y1[e] += eh * (g1[e] - wb[e]);
    }
  };
  // H = -log p + D/2 log 2 pi + 1/2 log|G| + 1/2 m^T G^-1 m  (S:731)   (rmhmc_fused_kernel: hamiltonian, series branch)
  auto hamiltonian = [&](uint32_t n, uint32_t sub, const T (&X)[4], const T* m, const T (&mr)[4], T& H, T& logp, T (&Pd_out)[4],
                         T (&Sm_out)[4]) {
    T* d = (dpar && !TRACK) ? t.D1 : t.D0;                  // (TRACK: D1 belongs to the refresh phase)
    dpar ^= 1;
    jitter4(n, sub);
    T dr[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) dr[e] = t.rok[e] ? X[e] - t.mu_r[e] : 0.f;
    t.put4(t.EV, ev_r);
    t.put4(d, dr);
    __syncthreads();
    bf4 Pd = {0.f, 0.f, 0.f, 0.f}, x0v = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    t.prod2(t.Pa, d, t.Sa, m, Pd, x0v);
    if (a.has_jitter) t.prod1_sq(t.EV, s2);                 // second-order log-det term: (S . S) e
    T v[3] = {0.f, 0.f, 0.f}, x0[4], xr[4], wv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x0[e] = x0v[e]; xr[e] = x0v[e];
      Pd_out[e] = Pd[e]; Sm_out[e] = x0v[e];
      v[0] += dr[e] * Pd[e];
      wv[e] = ev_r[e] * x0v[e];
      if (a.has_jitter) v[2] += ev_r[e] * (t.sd_r[e] - 0.5f * s2[e]);    // log|P + E| = log|P| + tr(SE) - 1/2 tr((SE)^2) + ...
    }
    t.put4(t.W0, wv);
    refine(x0, xr);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[1] += mr[e] * xr[e];
    t.block_sums(v);
    const float pi_term = (float)D * 1.8378770351409912f;   // S:712
    logp = a.log_norm - 0.5f * v[0];
    H = -logp + 0.5f * pi_term + 0.5f * (a.logdetP + v[2]) + 0.5f * v[1];
  };

  const int row0 = t.row0;
  const int64_t ngroup = (a.C + Tile::NC - 1) / Tile::NC;
  for (int64_t cg = blockIdx.x; cg < ngroup; cg += gridDim.x) {
    const int64_t c = Tile::NC * cg + t.cl;
    live = c < a.C;
    chain = a.chain_offset + (uint64_t)(live ? c : 0);
    T scur[4], sth[4], spm[4], sthc[4], spmc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) scur[e] = (live && t.rok[e]) ? a.cur[c * D + row0 + e] : 0.f;
    int32_t rejected = 0;
    __syncthreads();                                        // the previous group's last reads of the vector matrices
    for (int tr = 0; tr < a.n_traj; ++tr) {
      const uint32_t n = (uint32_t)(a.traj_offset + tr);
      // ---- gibbs: p = chol(G(theta)) z, drawn ahead by the momentum kernel (S:183-184)
#pragma unroll
      for (int e = 0; e < 4; ++e) spm[e] = (live && t.rok[e]) ? a.p_ws[((int64_t)tr * a.C + c) * D + row0 + e] : 0.f;
      t.put4(t.PM, spm);
      T H0, H1, lp0, lp1;
      hamiltonian(n, 1, scur, t.PM, spm, H0, lp0, y, z);    // S:971 -> S:822
#pragma unroll
      for (int e = 0; e < 4; ++e) { sth[e] = scur[e]; sthc[e] = scur[e]; spmc[e] = spm[e]; yc[e] = y[e]; zc[e] = z[e]; }   // S:425-426
      if (!TRACK) t.put4(t.PMC, spm);
      for (int lstep = 0; lstep < a.L; ++lstep) {           // S:427-461
        const uint32_t k0 = 2u + 8u * (uint32_t)lstep;
        if (TRACK) pair_tracked(t.WSA, n, k0 + 1, k0 + 2, sth, sthc, spm, spmc, y, yc, z, zc);    // phi_A/2, phi_B/2  S:429-433
        else {
          half_step(n, k0 + 1, sth, t.PMC, sthc, spm, t.PM);    // phi_A/2  S:429-430
          half_step(n, k0 + 2, sthc, t.PM, sth, spmc, t.PMC);   // phi_B/2  S:432-433
        }
        if (a.K == 0) __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {                       // phi_C    S:447-450, sequential (Q1)
          T xx = sth[e], b = spm[e], xc = sthc[e], bc = spmc[e];
          const T h = 0.5f, cc = a.rot_c, ss = a.rot_s;
          xx = h * ((xx + xc) + cc * (xx - xc) + ss * (b - bc));
          b = h * ((b + bc) - ss * (xx - xc) + cc * (b - bc));
          xc = h * ((xx + xc) - cc * (xx - xc) - ss * (b - bc));
          bc = h * ((b + bc) + ss * (xx - xc) - cc * (b - bc));
          sth[e] = xx; spm[e] = b; sthc[e] = xc; spmc[e] = bc;
        }
        t.put4(t.PM, spm);
        t.put4(t.PMC, spmc);
        if (TRACK) {                                        // the four tracked products of the rotated state, afresh
          T dt[4], dc[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) { dt[e] = t.rok[e] ? sth[e] - t.mu_r[e] : 0.f; dc[e] = t.rok[e] ? sthc[e] - t.mu_r[e] : 0.f; }
          t.put4(t.D1, dt);
          t.put4(t.DC, dc);
          __syncthreads();
          bf4 p1 = {0.f, 0.f, 0.f, 0.f}, p2 = {0.f, 0.f, 0.f, 0.f}, s3 = {0.f, 0.f, 0.f, 0.f}, s4 = {0.f, 0.f, 0.f, 0.f};
          t.prod4(t.D1, t.DC, t.PM, t.PMC, p1, p2, s3, s4);
#pragma unroll
          for (int e = 0; e < 4; ++e) { y[e] = p1[e]; yc[e] = p2[e]; z[e] = s3[e]; zc[e] = s4[e]; }
          pair_tracked(t.WSB, n, k0 + 4, k0 + 7, sthc, sth, spmc, spm, yc, y, zc, z);   // phi_B/2, phi_A/2  S:454-458
        } else {
          half_step(n, k0 + 4, sthc, t.PM, sth, spmc, t.PMC);   // phi_B/2  S:454-455
          half_step(n, k0 + 7, sth, t.PMC, sthc, spm, t.PM);    // phi_A/2  S:457-458
        }
      }
      if (TRACK) {                                          // (the tracked half steps keep the momenta in registers)
        if (a.K == 0) __syncthreads();                      // no solve phase since the refresh phase read PM
        t.put4(t.PM, spm);
      }
      T unused1[4], unused2[4];
      hamiltonian(n, 2u + 8u * (uint32_t)a.L, sth, t.PM, spm, H1, lp1, unused1, unused2);   // S:989 (Q4)
      // ---- Metropolis test + bookkeeping (S:1000-1026, S:1045-1057)
      const T u = u23<T>(philox_block(a.seed, chain, n, PURPOSE_MH, 0, 0).x);
      const bool acc = mh_accept<T>(H0, H1, lp1, u);
      const bool reset = (!acc) && ((int)n == a.burn + 1);  // Q2
      if (live) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (t.rok[e]) {
            const T vnew = acc ? sth[e] : (reset ? a.theta_init[c * D + row0 + e] : scur[e]);
            scur[e] = vnew;
            if (a.samples && (int)n > a.burn) a.samples[((int64_t)((int)n - a.burn) * a.C + c) * D + row0 + e] = vnew;
          }
        }
        if (t.writer) {
          if (a.H_old) a.H_old[(int64_t)tr * a.C + c] = H0;
          if (a.H_new) a.H_new[(int64_t)tr * a.C + c] = H1;
          if (a.accept) a.accept[(int64_t)tr * a.C + c] = acc ? 1 : 0;
        }
      }
      if (!acc) ++rejected;
    }
    if (live) {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (t.rok[e]) a.cur[c * D + row0 + e] = scur[e];
      if (t.writer) a.reject_count[c] += rejected;
    }
  }
}

}  // namespace hta
