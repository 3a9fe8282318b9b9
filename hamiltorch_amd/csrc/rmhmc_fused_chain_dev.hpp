// rmhmc_fused.hip, device side 2 of 4: one chain (or two) per workgroup of 256 threads - the register-resident slices of P and S and
// their products (Fused), the whole run of a chain (fused_body) and its kernels, rmhmc_fused_kernel (two workgroups per CU) and
// rmhmc_fused_kernel_wide (one).  The launcher and the mathematics behind the route: the head of rmhmc_fused.hip.
#pragma once
#include <utility>
#include "philox.hpp"
#include "rmhmc_fused_dev.hpp"
#include "rmhmc_fused_chol_dev.hpp"

namespace hta {

// Sum of the two half-row partials of a row: lanes l (lower k half) and l + 32 (upper half) of one wave.  The total is
// valid in the UPPER lane (the row's owner).  v_permlane32_swap_b32 (gfx950) puts the lower half of `h` under the upper
// lanes in one VALU op - an LDS bpermute round trip here costs more than the barrier it saves.
__device__ __forceinline__ float row_total(float h) {
  const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, h), __builtin_bit_cast(unsigned, h), false, false);
  return h + __builtin_bit_cast(float, r[0]);
}
__device__ __forceinline__ double row_total(double h) { return h + __shfl_xor(h, 32, 64); }

// acc += s * (lane J of this lane's 16-lane row of u): v_fmac_f32 with the DPP row_newbcast control (gfx90a+).  A chunk of
// 16 vector elements then costs ONE 4-byte LDS load per lane (lane l fetches element l & 15) and 16 FMAs, instead of four
// 16-byte loads that every lane repeats: the product passes were LDS-bandwidth bound (8 clocks per 16-byte wave load).
template <int J> __device__ __forceinline__ void fmac_bcast(float& acc, float u, float s) {
  asm("v_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(u), "v"(s), "n"(J));
}
template <int... J>
__device__ __forceinline__ void chunk_fma(const float* reg, float u, float (&acc)[2], std::integer_sequence<int, J...>) {
  (fmac_bcast<J>(acc[J & 1], u, reg[J]), ...);
}

// KH: register-resident slice of a matrix column per thread (multiple of 8).  Lane (row, half) keeps P[k][row] and
// S[k][row] for its KH values of k in VGPRs for the whole launch; a matrix-vector product then only streams the
// vector (16-byte LDS reads).  The two halves of a row sit in the SAME wave (lanes l and l + 32): their partial sums
// meet through one lane swap, the upper lane ("owner" of the row) finishes the element-wise work of its element in
// registers - no partial-sum vectors, no combine phases: one barrier per product pass.
// NC chains can share a workgroup (NC = 2): the slices do not depend on the chain, so a pass carries both chains for the
// same register reads and barriers - but not for the same LDS traffic, which is what bounds a pass (see the dispatch).
constexpr int FVC = 16;           // LDS vectors per chain: pm pmc ev d0 d1 w0 w1 | dc + 8 solve vectors of the tracked schedule
                                  // (128 entries each, zero beyond D)

// The kernel's LDS block, offsets in elements of T: NC x FVC vectors | dg[128] | red[32] | jb[8 evaluation slots][128] | W[D][ld], the
// Cholesky work matrix (need_w only).  fused_body carves with it, the launcher sizes with it (fused_lds_bytes).
struct FusedLds {
  int dg, red, jb, W;
  size_t elems;
  __host__ __device__ constexpr FusedLds(int NC, int D, int ld, bool need_w)
      : dg(NC * FVC * 128), red(dg + 128), jb(red + 32), W(jb + 8 * 128), elems((size_t)W + (need_w ? (size_t)D * ld : 0)) {}
};

template <typename T, int KH, int NC, bool TRACK = false> struct Fused {
  typedef T V4 __attribute__((ext_vector_type(4)));
  static constexpr int CHS = FVC * 128;
  const FusedArgs<T>& a;
  int D, ld, tid, row, k0, dpar;
  bool own;
  T Preg[KH], Sreg[KH];
  T mu_r, sd_r;                       // mu[row], S[row][row]
  T ev_r[NC];                         // this owner's elements of the current evaluation's jitter
  T scur[NC], sth[NC], spm[NC], sthc[NC], spmc[NC];   // the owner's element of the chain state (theta, p and their copies):
                                      // registers; only the momenta are mirrored in LDS (they are product operands)
  int jslot;                          // next unread evaluation slot of the jitter buffer
  T y[NC], yc[NC], z[NC], zc[NC];     // TRACK: the owner's element of P (theta - mu), P (theta_c - mu), S p, S p_c
  T *pm, *pmc, *ev, *d0, *d1, *w0, *w1, *dc, *ws, *dg, *red, *W, *jb;
  uint64_t chain[NC];
  bool live[NC];
  __device__ Fused(const FusedArgs<T>& a_) : a(a_) {}

  __device__ __forceinline__ void load_slices() {           // once per launch (symmetric matrices: column `row`)
    const bool rowok = row < D;
#pragma unroll
    for (int kk = 0; kk < KH; ++kk) {
      const int k = k0 + kk;
      const bool ok = rowok && k < D;
      Preg[kk] = ok ? a.P[(int64_t)k * D + row] : (T)0;
      Sreg[kk] = ok ? a.S[(int64_t)k * D + row] : (T)0;
    }
  }

  // NC x 4 block sums at once (every thread gets all of them)
  __device__ __forceinline__ void block_sums(T (&v)[NC][4]) {
#pragma unroll
    for (int q = 0; q < NC; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[q][e] = wave_sum(v[q][e]);
    __syncthreads();
    if ((tid & 63) == 0) {
#pragma unroll
      for (int q = 0; q < NC; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[(tid >> 6) * 8 + q * 4 + e] = v[q][e];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NC; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        T s = 0;
#pragma unroll
        for (int i = 0; i < FNT / 64; ++i) s += red[i * 8 + q * 4 + e];
        v[q][e] = s;
      }
  }

  // Row `row` of up to three symmetric-matrix x vector products per chain, complete in both lanes of the row:
  //   o1 = P v1,  o2 = S v2,  o3 = (S . S) v3  (element-wise square: the second-order log-det term).
  // No barriers inside; vectors and slices are zero beyond D.
  template <bool WITH_P, int NS>
  __device__ __forceinline__ void products(const T* v1, const T* v2, const T* v3, T (&o1)[NC], T (&o2)[NC], T (&o3)[NC]) {
    T a1[NC][2], a2[NC][2], a3[NC][2];
#pragma unroll
    for (int q = 0; q < NC; ++q) { a1[q][0] = a1[q][1] = a2[q][0] = a2[q][1] = a3[q][0] = a3[q][1] = 0; }
    constexpr int NCH = KH / 4;
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      if (NS <= 1 && sizeof(T) == 4) {
        // fp32: one 4-byte load per lane and chunk of 16 elements, broadcast inside the FMA (see fmac_bcast)
        constexpr int NB = (KH + 15) / 16;
        float u1[NB], u2[NB];
        const int l15 = tid & 15;
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
          const int off = q * CHS + k0 + 16 * cb + ((16 * cb + 8 < KH) ? l15 : (l15 & 7));    // a trailing half chunk has 8 elements
          if (WITH_P) u1[cb] = v1[off];
          if (NS >= 1) u2[cb] = v2[off];
        }
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
          if (16 * cb + 8 < KH) {
            if (WITH_P) chunk_fma(reinterpret_cast<const float*>(Preg) + 16 * cb, u1[cb], reinterpret_cast<float(&)[2]>(a1[q]), std::make_integer_sequence<int, 16>{});
            if (NS >= 1) chunk_fma(reinterpret_cast<const float*>(Sreg) + 16 * cb, u2[cb], reinterpret_cast<float(&)[2]>(a2[q]), std::make_integer_sequence<int, 16>{});
          } else {
            if (WITH_P) chunk_fma(reinterpret_cast<const float*>(Preg) + 16 * cb, u1[cb], reinterpret_cast<float(&)[2]>(a1[q]), std::make_integer_sequence<int, 8>{});
            if (NS >= 1) chunk_fma(reinterpret_cast<const float*>(Sreg) + 16 * cb, u2[cb], reinterpret_cast<float(&)[2]>(a2[q]), std::make_integer_sequence<int, 8>{});
          }
        }
      } else if (NS <= 1) {
        // every 16-byte vector load of this chain first, then the FMAs: left to itself the compiler issues three loads
        // and waits for them, 14 exposed LDS round trips per pass
        V4 u1[NCH], u2[NCH];
#pragma unroll
        for (int cb = 0; cb < NCH; ++cb) {
          if (WITH_P) u1[cb] = *reinterpret_cast<const V4*>(v1 + q * CHS + k0 + 4 * cb);
          if (NS >= 1) u2[cb] = *reinterpret_cast<const V4*>(v2 + q * CHS + k0 + 4 * cb);
        }
#pragma unroll
        for (int cb = 0; cb < NCH; ++cb) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (WITH_P) a1[q][e & 1] = fma(Preg[4 * cb + e], u1[cb][e], a1[q][e & 1]);
            if (NS >= 1) a2[q][e & 1] = fma(Sreg[4 * cb + e], u2[cb][e], a2[q][e & 1]);
          }
        }
      } else {
#pragma unroll
        for (int kk = 0; kk < KH; kk += 4) {
          V4 u1, u2, u3;
          if (WITH_P) u1 = *reinterpret_cast<const V4*>(v1 + q * CHS + k0 + kk);
          u2 = *reinterpret_cast<const V4*>(v2 + q * CHS + k0 + kk);
          u3 = *reinterpret_cast<const V4*>(v3 + q * CHS + k0 + kk);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (WITH_P) a1[q][e & 1] = fma(Preg[kk + e], u1[e], a1[q][e & 1]);
            a2[q][e & 1] = fma(Sreg[kk + e], u2[e], a2[q][e & 1]);
            a3[q][e & 1] = fma(Sreg[kk + e] * Sreg[kk + e], u3[e], a3[q][e & 1]);
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      if (WITH_P) o1[q] = row_total(a1[q][0] + a1[q][1]);
      if (NS >= 1) o2[q] = row_total(a2[q][0] + a2[q][1]);
      if (NS >= 2) o3[q] = row_total(a3[q][0] + a3[q][1]);
    }
  }

  __device__ __forceinline__ T jitter_elem(int q, uint32_t n, uint32_t sub) {
    return (a.has_jitter && own && live[q]) ? a.jitter * uniform_elem<T>(a.seed, chain[q], n, PURPOSE_JITTER, sub, row) : (T)0;
  }

  // Jitter of the next NSLOT evaluations of the integrator in ONE Philox pass per wave: lane (slot, blk) draws the block
  // of 4 uniforms of rows 32 wave + 4 blk .. + 3 for evaluation `slot` (NC == 1: 8 evaluations = 2 steps; NC == 2: 4
  // evaluations x 2 chains = 1 step).  A wave only ever reads the rows it wrote: no barrier.  (Drawing per evaluation
  // costs ~100 VALU instructions per wave and half step however few lanes need it - a fifth of the half step.)
  static constexpr int NSLOT = 8 / NC;
  __device__ __forceinline__ void refill_jitter(uint32_t n, int l) {
    jslot = 0;
    if (!a.has_jitter) return;
    const int lane = tid & 63, slot = lane >> 3, blk = lane & 7;
    const int q = NC == 1 ? 0 : (slot & 1), e = NC == 1 ? slot : (slot >> 1);
    const int which = e & 3;
    const uint32_t sub = 2u + 8u * (uint32_t)(l + (e >> 2)) + (which == 0 ? 1u : which == 1 ? 2u : which == 2 ? 4u : 7u);
    const int r0 = 32 * (tid >> 6) + 4 * blk;
    const U4 r = philox_block(a.seed, chain[q], n, PURPOSE_JITTER, sub, (uint32_t)(r0 >> 2));
    const V4 val = {a.jitter * u23<T>(r.x), a.jitter * u23<T>(r.y), a.jitter * u23<T>(r.z), a.jitter * u23<T>(r.w)};
    *reinterpret_cast<V4*>(jb + (e * NC + q) * 128 + r0) = val;
  }

  // x = (P + diag(e))^-1 m continued from x0 = S m: xr <- x0 - S (e . x), K times; w buffers alternate (a fast wave's
  // store of the next e . x must not overtake a slow wave's reads of the current one)
  __device__ __forceinline__ void refine(const T (&x0)[NC], T (&xr)[NC]) {
    for (int it = 0; it < a.K; ++it) {
      const T* wr = (it & 1) ? w1 : w0;
      T* ww = (it & 1) ? w0 : w1;
      __syncthreads();
      T sx[NC], u1[NC], u3[NC];
      products<false, 1>(nullptr, wr, nullptr, u1, sx, u3);
      if (own) {
#pragma unroll
        for (int q = 0; q < NC; ++q) { xr[q] = x0[q] - sx[q]; ww[q * CHS + row] = ev_r[q] * xr[q]; }
      }
    }
  }

  // one half step (csrc/rmhmc_explicit.hip:half_step): upd_x += eh G(X)^-1 m ; upd_g -= eh P (X - mu); its jitter is
  // the next slot of the buffer refill_jitter() filled.  X, upd_x: owner registers; m: LDS vector; upd_g: owner register
  // mirrored to its LDS vector.  1 + K barriers.
  __device__ __forceinline__ void half_step(const T (&X)[NC], const T* m, T (&upd_x)[NC], T (&upd_g)[NC], T* upd_g_lds, T eh) {
    T* d = dpar ? d1 : d0;                                 // alternate: with K == 0 nothing else separates two evaluations
    dpar ^= 1;
    if (own) {
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        ev_r[q] = a.has_jitter ? jb[(jslot * NC + q) * 128 + row] : (T)0;
        d[q * CHS + row] = X[q] - mu_r;
      }
    }
    ++jslot;
    __syncthreads();
    T Pd[NC], x0[NC], u3[NC], xr[NC];
    products<true, 1>(d, m, nullptr, Pd, x0, u3);
    if (own) {
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        upd_g[q] -= eh * Pd[q];
        upd_g_lds[q * CHS + row] = upd_g[q];
        xr[q] = x0[q];
        w0[q * CHS + row] = ev_r[q] * x0[q];
      }
    }
    refine(x0, xr);
    if (own) {
#pragma unroll
      for (int q = 0; q < NC; ++q) upd_x[q] += eh * xr[q];
    }
  }

  // ---- TRACK: the half steps without their P d and S m products (the schedule and its derivation: rows4_trajectories) ----
  // Up to two P products and two S products with ONE pass over the slices: op_i = P vp_i, os_i = S vs_i, complete in both
  // lanes of the row.  Per product the chunks and the order of the sum are those of products().
  template <int NPV, int NSV>
  __device__ __forceinline__ void products_multi(const T* vp0, const T* vp1, const T* vs0, const T* vs1, T (&op0)[NC], T (&op1)[NC],
                                                 T (&os0)[NC], T (&os1)[NC]) {
    constexpr int NV = NPV + NSV;
    const T* vec[4] = {vp0, vp1, vs0, vs1};
    T acc[NC][4][2];
#pragma unroll
    for (int q = 0; q < NC; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[q][i][0] = acc[q][i][1] = 0;
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      if constexpr (sizeof(T) == 4) {
        constexpr int NB = (KH + 15) / 16;
        float u[4][NB];
        const int l15 = tid & 15;
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
          const int off = q * CHS + k0 + 16 * cb + ((16 * cb + 8 < KH) ? l15 : (l15 & 7));
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool used = i < 2 ? i < NPV : i - 2 < NSV;
            if (used) u[i][cb] = vec[i][off];
          }
        }
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool used = i < 2 ? i < NPV : i - 2 < NSV;
            if (!used) continue;
            const float* reg = reinterpret_cast<const float*>(i < 2 ? Preg : Sreg) + 16 * cb;
            if (16 * cb + 8 < KH) chunk_fma(reg, u[i][cb], reinterpret_cast<float(&)[2]>(acc[q][i]), std::make_integer_sequence<int, 16>{});
            else chunk_fma(reg, u[i][cb], reinterpret_cast<float(&)[2]>(acc[q][i]), std::make_integer_sequence<int, 8>{});
          }
        }
      } else {
        constexpr int NCH = KH / 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool used = i < 2 ? i < NPV : i - 2 < NSV;
          if (!used) continue;
          V4 uu[NCH];
#pragma unroll
          for (int cb = 0; cb < NCH; ++cb) uu[cb] = *reinterpret_cast<const V4*>(vec[i] + q * CHS + k0 + 4 * cb);
#pragma unroll
          for (int cb = 0; cb < NCH; ++cb)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[q][i][e & 1] = fma((i < 2 ? Preg : Sreg)[4 * cb + e], uu[cb][e], acc[q][i][e & 1]);
        }
      }
    }
    (void)NV;
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      if (NPV >= 1) op0[q] = row_total(acc[q][0][0] + acc[q][0][1]);
      if (NPV >= 2) op1[q] = row_total(acc[q][1][0] + acc[q][1][1]);
      if (NSV >= 1) os0[q] = row_total(acc[q][2][0] + acc[q][2][1]);
      if (NSV >= 2) os1[q] = row_total(acc[q][3][0] + acc[q][3][1]);
    }
  }

  // two independent solves x = (P + E)^-1 m from x_0 = S m, K phases (one barrier and one pass over S each); wa / wb return
  // e . x_(K-1) (zero without jitter).  wb4: this pair's four vectors a0 a1 b0 b1.
  __device__ __forceinline__ void solve2(T* wb4, const T (&ea)[NC], const T (&eb)[NC], const T (&x0a)[NC], const T (&x0b)[NC],
                                         T (&xa)[NC], T (&xb)[NC], T (&wa)[NC], T (&wb)[NC]) {
#pragma unroll
    for (int q = 0; q < NC; ++q) { xa[q] = x0a[q]; xb[q] = x0b[q]; wa[q] = 0; wb[q] = 0; }
    for (int it = 0; it < a.K; ++it) {
      T* A = wb4 + (it & 1) * 128;                         // read in this phase only; rewritten two phases later
      T* B = A + 2 * 128;
      if (own) {
#pragma unroll
        for (int q = 0; q < NC; ++q) {
          wa[q] = ea[q] * xa[q]; wb[q] = eb[q] * xb[q];
          A[q * CHS + row] = wa[q]; B[q * CHS + row] = wb[q];
        }
      }
      __syncthreads();
      T ra[NC], rb[NC], u0[NC], u1[NC];
      products_multi<0, 2>(nullptr, nullptr, A, B, u0, u1, ra, rb);
#pragma unroll
      for (int q = 0; q < NC; ++q) { xa[q] = x0a[q] - ra[q]; xb[q] = x0b[q] - rb[q]; }
    }
  }

  // a pair of half steps (S:429-433 and, with the roles of the copies swapped, S:454-458):
  //   a:  g1 -= eh P (X1 - mu)   X2 += eh (P + E_a)^-1 g2        b:  g2 -= eh P (X2 - mu)   X1 += eh (P + E_b)^-1 g1
  // with y1 = P (X1 - mu), y2 = P (X2 - mu), z1 = S g1, z2 = S g2 kept current; the jitter of a and b: the next two slots
  __device__ __forceinline__ void pair_tracked(T* wb4, T (&X1)[NC], T (&X2)[NC], T (&g1)[NC], T (&g2)[NC], T (&y1)[NC], T (&y2)[NC],
                                               T (&z1)[NC], T (&z2)[NC], T eh) {
    T ea[NC], eb[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      ea[q] = (a.has_jitter && own) ? jb[(jslot * NC + q) * 128 + row] : (T)0;
      eb[q] = (a.has_jitter && own) ? jb[((jslot + 1) * NC + q) * 128 + row] : (T)0;
      g1[q] -= eh * y1[q];                                  // a's momentum update ...
      z1[q] -= eh * (X1[q] - mu_r);                         // ... and S g1 with it (S P = I)
    }
    jslot += 2;
    T xa[NC], xb[NC], wa[NC], wb[NC];
    solve2(wb4, ea, eb, z2, z1, xa, xb, wa, wb);
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      X2[q] += eh * xa[q];                                  // a's position update; P x_a = g2 - e_a . x_a(K-1)
      y2[q] += eh * (g2[q] - wa[q]);
      g2[q] -= eh * y2[q];                                  // b's momentum update
      z2[q] -= eh * (X2[q] - mu_r);
      X1[q] += eh * xb[q];                                  // b's position update
      y1[q] += eh * (g1[q] - wb[q]);
    }
  }

  // the four tracked products of the current state, afresh (after the rotation phi_C): one barrier, one pass over P and S
  __device__ __forceinline__ void refresh_tracked() {
    if (own) {
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        d1[q * CHS + row] = sth[q] - mu_r; dc[q * CHS + row] = sthc[q] - mu_r;
        pm[q * CHS + row] = spm[q]; pmc[q * CHS + row] = spmc[q];
      }
    }
    __syncthreads();
    products_multi<2, 2>(d1, dc, pm, pmc, y, yc, z, zc);
  }

  __device__ __forceinline__ T factor() { return chol_in_lds<T>(a.P, ev, W, dg, D, ld, tid); }

  // H = -log p + D/2 log 2 pi + 1/2 log|G| + 1/2 m^T G^-1 m  (S:731) at (X, m) per chain, jitter sub-stream `sub`
  __device__ __forceinline__ void hamiltonian(uint32_t n, uint32_t sub, const T (&X)[NC], const T* m, const T (&mr)[NC], T (&H)[NC],
                                              T (&logp)[NC], T (&Pd_out)[NC], T (&Sm_out)[NC]) {
    T* d = (dpar && !TRACK) ? d1 : d0;                      // (TRACK: d1 belongs to the refresh phase)
    dpar ^= 1;
    T dr[NC];
    if (own) {
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        const T e = jitter_elem(q, n, sub);
        ev_r[q] = e; ev[q * CHS + row] = e;
        dr[q] = X[q] - mu_r; d[q * CHS + row] = dr[q];
      }
    }
    const bool series = a.series || !a.has_jitter;
    T ld_exact = 0;
    if (NC == 1 && !series) ld_exact = factor();              // exact log|P + E| (its own barriers; reads ev from LDS)
    __syncthreads();
    T Pd[NC], x0[NC], s2[NC], xr[NC];
    if (series && a.has_jitter) products<true, 2>(d, m, ev, Pd, x0, s2);
    else products<true, 1>(d, m, nullptr, Pd, x0, s2);
    T v[NC][4];
#pragma unroll
    for (int q = 0; q < NC; ++q) { v[q][0] = v[q][1] = v[q][2] = v[q][3] = 0; xr[q] = x0[q]; Pd_out[q] = Pd[q]; Sm_out[q] = x0[q]; }
    if (own) {
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        v[q][0] = dr[q] * Pd[q];
        w0[q * CHS + row] = ev_r[q] * x0[q];
        // log|P + E| = log|P| + tr(SE) - 1/2 tr((SE)^2) + O(D rho^3 / 3)
        if (series && a.has_jitter) v[q][2] = ev_r[q] * (sd_r - (T)0.5 * s2[q]);
      }
    }
    if (NC == 1 && !series) v[0][2] = ld_exact;
    refine(x0, xr);
    if (own) {
#pragma unroll
      for (int q = 0; q < NC; ++q) v[q][1] = mr[q] * xr[q];
    }
    block_sums(v);
    const float pi_term = (float)D * 1.8378770351409912f;     // S:712: float32 whatever the state dtype
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const T lp = a.log_norm - (T)0.5 * v[q][0];
      const T logdet = series ? a.logdetP + v[q][2] : v[q][2];
      logp[q] = lp;
      H[q] = -lp + (T)0.5 * (T)pi_term + (T)0.5 * logdet + (T)0.5 * v[q][1];
    }
  }
};

template <typename T, int KH, int NC, bool TRACK = false>
__device__ __forceinline__ void fused_body(const FusedArgs<T>& a, int ld, int need_w) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  typedef Fused<T, KH, NC, TRACK> F;
  F ch(a);
  const int D = a.D, tid = threadIdx.x;
  ch.D = D; ch.ld = ld; ch.tid = tid; ch.dpar = 0;
  {
    const int wave = tid >> 6, lane = tid & 63;
    ch.row = 32 * wave + (lane & 31);
    ch.k0 = (lane >> 5) ? KH : 0;
    ch.own = (lane >= 32) && ch.row < D;                    // the upper lane of a row holds the complete sums
  }
  T* v = reinterpret_cast<T*>(smem_raw);
  T** slots[9] = {&ch.pm, &ch.pmc, &ch.ev, &ch.d0, &ch.d1, &ch.w0, &ch.w1, &ch.dc, &ch.ws};    // ws: 8 vectors
  for (int i = 0; i < 9; ++i) *slots[i] = v + i * 128;
  constexpr FusedLds lay(NC, 0, 0, false);                  // (the offsets depend on NC alone)
  ch.dg = v + lay.dg;
  ch.red = v + lay.red;
  ch.jb = v + lay.jb;
  ch.W = v + lay.W;                                         // only with need_w
  for (int e = tid; e < lay.red; e += FNT) v[e] = (T)0;     // the vectors and dg
  const int row = ch.row;
  ch.mu_r = row < D ? a.mu[row] : (T)0;
  ch.sd_r = row < D ? a.S[(int64_t)row * D + row] : (T)0;
  const T eh = (T)0.5 * a.eps;
  ch.load_slices();
  bool have_factor = false;                                 // without jitter chol(P) serves every chain and trajectory
  const int64_t ngroup = (a.C + NC - 1) / NC;
  for (int64_t cg = blockIdx.x; cg < ngroup; cg += gridDim.x) {
    int64_t c[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      c[q] = NC * cg + q;
      ch.live[q] = c[q] < a.C;                               // an odd chain count leaves the last pair half empty
      ch.chain[q] = a.chain_offset + (uint64_t)(ch.live[q] ? c[q] : 0);
    }
#pragma unroll
    for (int q = 0; q < NC; ++q) ch.scur[q] = (ch.own && ch.live[q]) ? a.cur[c[q] * D + row] : (T)0;
    int32_t rejected[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) rejected[q] = 0;
    for (int t = 0; t < a.n_traj; ++t) {
      const uint32_t n = (uint32_t)(a.traj_offset + t);
      // ---- gibbs: p = chol(G(theta)) z  (S:183-184), jitter sub-stream 0
      if (a.p_ws) {
        if (ch.own) {
#pragma unroll
          for (int q = 0; q < NC; ++q) {
            ch.spm[q] = ch.live[q] ? a.p_ws[((int64_t)t * a.C + c[q]) * D + row] : (T)0;
            ch.pm[q * F::CHS + row] = ch.spm[q];
          }
        }
      } else if (NC == 1) {                                   // no pre-drawn momenta: factor here (tid-indexed helper phases)
        // Not reached through the C ABI: rmhmc_explicit.hip always hands rmhmc_fused_sample room for at least four trajectories of
        // momenta (lending the augmented-state area if the workspace has none), so its `block` is > 0 and a.p_ws never null.  Kept:
        // taking the arm out changes the device code of every instance.  (Row tid of p = L z below: the twin of rmhmc_momentum_kernel's.)
        __syncthreads();
        if (tid < D) ch.ev[tid] = a.has_jitter ? a.jitter * uniform_elem<T>(a.seed, ch.chain[0], n, PURPOSE_JITTER, 0, tid) : (T)0;
        if (a.has_jitter || !have_factor) { ch.factor(); have_factor = true; }
        if (tid < D) ch.w1[tid] = normal_elem<T>(a.seed, ch.chain[0], n, 0, tid);
        __syncthreads();
        if (tid < D) {
          T acc0 = ch.dg[tid] * ch.w1[tid], acc1 = 0;
          const T* rowp = ch.W + tid * ld;
          int k = 0;
          for (; k + 1 < tid; k += 2) { acc0 = fma(rowp[k], ch.w1[k], acc0); acc1 = fma(rowp[k + 1], ch.w1[k + 1], acc1); }
          if (k < tid) acc0 = fma(rowp[k], ch.w1[k], acc0);
          ch.pm[tid] = acc0 + acc1;
        }
        __syncthreads();
        if (ch.own) ch.spm[0] = ch.pm[row];
      }
      // ---- H_old (S:971 -> S:822), sub-stream 1
      T H0[NC], H1[NC], lp0[NC], lp1[NC];
      ch.hamiltonian(n, 1, ch.scur, ch.pm, ch.spm, H0, lp0, ch.y, ch.z);
#pragma unroll
      for (int q = 0; q < NC; ++q) {                                          // S:425-426
        ch.sth[q] = ch.scur[q]; ch.sthc[q] = ch.scur[q]; ch.spmc[q] = ch.spm[q];
        ch.yc[q] = ch.y[q]; ch.zc[q] = ch.z[q];
        if (!TRACK && ch.own) ch.pmc[q * F::CHS + row] = ch.spm[q];
      }
      // ---- L explicit steps (S:427-461)
      for (int l = 0; l < a.L; ++l) {
        if (l == 0 || ch.jslot == F::NSLOT) ch.refill_jitter(n, l);         // sub-streams 2 + 8 l + {1, 2, 4, 7}, ...
        if (TRACK) ch.pair_tracked(ch.ws, ch.sth, ch.sthc, ch.spm, ch.spmc, ch.y, ch.yc, ch.z, ch.zc, eh);   // phi_A/2, phi_B/2  S:429-433
        else {
          ch.half_step(ch.sth, ch.pmc, ch.sthc, ch.spm, ch.pm, eh);           // phi_A/2  S:429-430
          ch.half_step(ch.sthc, ch.pm, ch.sth, ch.spmc, ch.pmc, eh);          // phi_B/2  S:432-433
        }
        if (a.K == 0) __syncthreads();                                        // slower waves may still stream pm (no refinement barrier)
#pragma unroll
        for (int q = 0; q < NC; ++q) {                                        // phi_C    S:447-450, sequential (Q1): phi_c_elem (rmhmc.hpp) by hand - the call moves the code object
          T xx = ch.sth[q], b = ch.spm[q], xc = ch.sthc[q], bc = ch.spmc[q];
          const T h = (T)0.5, cc = a.rot_c, ss = a.rot_s;
          xx = h * ((xx + xc) + cc * (xx - xc) + ss * (b - bc));
          b = h * ((b + bc) - ss * (xx - xc) + cc * (b - bc));
          xc = h * ((xx + xc) - cc * (xx - xc) - ss * (b - bc));
          bc = h * ((b + bc) + ss * (xx - xc) - cc * (b - bc));
          ch.sth[q] = xx; ch.spm[q] = b; ch.sthc[q] = xc; ch.spmc[q] = bc;
          if (!TRACK && ch.own) { ch.pm[q * F::CHS + row] = b; ch.pmc[q * F::CHS + row] = bc; }
        }
        if (TRACK) {
          ch.refresh_tracked();
          ch.pair_tracked(ch.ws + 4 * 128, ch.sthc, ch.sth, ch.spmc, ch.spm, ch.yc, ch.y, ch.zc, ch.z, eh);   // phi_B/2, phi_A/2  S:454-458
        } else {
          ch.half_step(ch.sthc, ch.pm, ch.sth, ch.spmc, ch.pmc, eh);          // phi_B/2  S:454-455
          ch.half_step(ch.sth, ch.pmc, ch.sthc, ch.spm, ch.pm, eh);           // phi_A/2  S:457-458
        }
      }
      if (TRACK) {                                                            // (the tracked half steps keep the momenta in registers)
        if (a.K == 0) __syncthreads();                                        // no solve phase since the refresh phase read pm
        if (ch.own) {
#pragma unroll
          for (int q = 0; q < NC; ++q) ch.pm[q * F::CHS + row] = ch.spm[q];
        }
      }
      // ---- H_new on the un-augmented pair (S:989, Q4), sub-stream 2 + 8L
      T unused1[NC], unused2[NC];
      ch.hamiltonian(n, 2u + 8u * (uint32_t)a.L, ch.sth, ch.pm, ch.spm, H1, lp1, unused1, unused2);
      // ---- Metropolis test + bookkeeping (S:1000-1026, S:1045-1057), as hmc_pieces.hip:mh_select_kernel
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        const T u = u23<T>(philox_block(a.seed, ch.chain[q], n, PURPOSE_MH, 0, 0).x);
        const bool acc = mh_accept<T>(H0[q], H1[q], lp1[q], u);
        const bool reset = (!acc) && ((int)n == a.burn + 1);                  // Q2
        if (ch.own && ch.live[q]) {
          const T vnew = acc ? ch.sth[q] : (reset ? a.theta_init[c[q] * D + row] : ch.scur[q]);
          ch.scur[q] = vnew;
          if (a.samples && (int)n > a.burn) a.samples[((int64_t)((int)n - a.burn) * a.C + c[q]) * D + row] = vnew;
        }
        if (!acc) ++rejected[q];
        if (tid == 0 && ch.live[q]) {
          if (a.H_old) a.H_old[(int64_t)t * a.C + c[q]] = H0[q];
          if (a.H_new) a.H_new[(int64_t)t * a.C + c[q]] = H1[q];
          if (a.accept) a.accept[(int64_t)t * a.C + c[q]] = acc ? 1 : 0;
        }
      }
    }
    if (ch.own) {
#pragma unroll
      for (int q = 0; q < NC; ++q) if (ch.live[q]) a.cur[c[q] * D + row] = ch.scur[q];
    }
    if (tid == 0) {
#pragma unroll
      for (int q = 0; q < NC; ++q) if (ch.live[q]) a.reject_count[c[q]] += rejected[q];
    }
  }
}

template <typename T, int KH, int NC, bool TRACK = false>
__global__ __launch_bounds__(FNT, 2) void rmhmc_fused_kernel(FusedArgs<T> a, int ld, int need_w) {
  fused_body<T, KH, NC, TRACK>(a, ld, need_w);
}

// The same kernel for launches of at most one workgroup per CU (chains <= compute units: BASELINE config 3's 256 chains):
// two workgroups per CU cannot be resident then, so the two-workgroup register cap of 256 - under which the KH = 56 / 64
// instances keep 26 / 35 registers in scratch - buys nothing.  kFusedWideVgprs registers instead: together with the
// overlapped momentum waves (rmhmc_momentum_wave_kernel, capped at 512 - kFusedWideVgprs) a SIMD's 512 are exactly used.
template <int KH, bool TRACK = false>
__global__ __launch_bounds__(FNT) __attribute__((amdgpu_num_vgpr(kFusedWideVgprs))) void rmhmc_fused_kernel_wide(FusedArgs<float> a, int ld, int need_w) {
  fused_body<float, KH, 1, TRACK>(a, ld, need_w);
}

}  // namespace hta
