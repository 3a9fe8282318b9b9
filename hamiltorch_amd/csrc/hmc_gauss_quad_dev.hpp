// Gaussian HMC, D <= 4, fp32: one chain per DPP quad - every launch form of the quad family (included by hmc_gaussian.hip).
#pragma once
#include <type_traits>
#include <utility>
#include "common.hpp"
#include "philox.hpp"
#include "hmc_gaussian.hpp"
#include "hmc_gauss_small_dev.hpp"
#include "quad_prop.hpp"

namespace hta {

// =============================================================================================
// D <= 4, fp32, identity mass, latency regime: one chain per DPP quad, one eigen-coordinate per lane
//
// In the eigenbasis the coordinates of a chain do not interact DURING a trajectory, so lane k of a quad integrates
// coordinate k alone: a step is the two dependent FMAs  y += eps r ; r -= eps lam_k y  and nothing else (the chain-per-lane
// kernel, hmc_gauss_eig_kernel in hmc_gauss_small_dev.hpp, issues four instructions per step at D = 3).  Lanes meet only at trajectory boundaries:
//   * accept test: h_old - h_new = sum_k (0.5 z_k^2 + 0.5 lam_k yc_k^2) - (0.5 r_k^2 + 0.5 lam_k y_k^2)  (log_norm cancels),
//     one two-stage quad butterfly (DPP quad_perm) of the per-lane difference; every lane gets the same decision;
//   * sample row: q_i = mu_i + sum_k Q[i][k] yc_k, lane i broadcasting yc_k from lane k (DPP quad_perm:[k,k,k,k]);
//   * the draw record [Q^T z, log u, pad] is read one element per lane; log u is lane D's element (D < 4).
// A lane >= D of the quad is a dummy coordinate (lam = 0, momentum 0).  1024 chains are 64 waves instead of 16; the
// dispatcher takes this kernel while the chip has idle SIMDs for the extra waves (C <= g_quad_max_chains) and the
// chain-per-lane kernel beyond, where instruction count per chain decides.
// =============================================================================================
constexpr int QUAD_FUSED_NS = 4;               // record look-ahead of the fused, local and wide launches (trajectories)
constexpr int QUAD_SLOTS = 4;                  // deepest record look-ahead of the quad kernels = rows of slack in the workspace
template <int CTRL> __device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
template <int K> __device__ __forceinline__ float quad_bcast(float v) { return dpp_f<K * 0x55>(v); }
__device__ __forceinline__ float quad_sum(float v) {
  v += dpp_f<0xB1>(v);          // quad_perm:[1,0,3,2]
  v += dpp_f<0x4E>(v);          // quad_perm:[2,3,0,1]
  return v;
}

// LB > 0: a.L == LB is known at compile time (straight-line steps, no loop bookkeeping: at this size every scalar
// instruction on the hot path costs what a vector one does); LB == 0: any L.
//
// VAR (tuning key "quad_variant", default 7) - the same arithmetic, fewer instructions around it (a lone wave pays ~2 ns for
// ANY instruction, so the 28 that are not the trajectory's 52 dependent FMAs are a third of its time):
//   bit 0  addresses as a wave-uniform base (an SGPR pair, advanced once per pass of the unrolled loop) plus a 32-bit lane
//          offset per position of that loop (loop-invariant registers): no 64-bit vector add per record load and per row store
//          (the VAR = 0 loop spends 27 of its 320 instructions per four trajectories on address arithmetic, this one 8);
//   bit 1  no NaN guard in front of the accept compare: the record's 2 log u is finite by construction (u23: 23-bit uniforms
//          in (0, 1)), the energy difference is finite, -inf or NaN (sums of squares cannot reach -inf, the current point is
//          finite), and both -inf >= x and NaN >= x are false - the guard never changes a decision.
//   bit 2  the row element and the quad butterfly of the energy difference as ONE interleaved block (see TAIL below).
// Results are bit-identical to VAR = 0 (tests/test_gpu_hmc.py::test_quad_kernel_variants_are_bit_identical).  Measured at BASELINE
// config 2 (profiles/r03v_*): 166.3 us (VAR 0) -> 157.5 us (VAR 7) per 1000-trajectory launch; the static count 78.5 -> 73.25
// instructions per trajectory (tools/isa_of.py --loops) predicted 155.  With 16 trajectories per pass at L = 25: 72.6, 156.6 us.
template <int I, int N, typename F> __device__ __forceinline__ void quad_static_for(F&& f) {
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); quad_static_for<I + 1, N>(f); }
}
// FUSED (round 4, tuning key "quad_fused"): the pre-draw pass runs INSIDE the same launch - the blocks behind the consumers' are
// producers (quad_fused_kernel below) that write the records chunk by chunk (CH whole trajectories: no 128-byte line straddles two
// chunks) and count themselves into `flags[chunk]` with a release at agent scope; a consumer checks, once per pass of its unrolled
// loop, that the rows the pass prefetches are complete (`ready`: a register compare), polling a chunk's counter only when it
// crosses into that chunk, with the next chunk's counter requested one chunk ahead.  Same records, same arithmetic: results are
// bit-identical to the two-launch form.
// HAND-OVER FAILURE (round 5).  The consumers wait for producers of the SAME grid: that is safe only while both are resident, which
// a launch of 80-320 blocks on an idle 256-CU chip is, and a shared or preempted GPU need not be.  The wait is bounded; a consumer
// whose bound expires does NOT read on (round 4 did: plausible, wrong samples with rc 0): it raises the workspace's STICKY status
// word (`err`: set with an atomic OR, zeroed only by hta_hmc_gaussian_prepare, readable by the host at the byte offset
// hta_hmc_gaussian_status_offset returns), stops waiting, and when its trajectories are done overwrites every row it stored in this
// launch and its slot of the chain state with NaN - the failure is in the data as well as in the word.  All of it is off the hot
// path (inside the once-per-chunk poll and after the loops).  Debug key "quad_starve" makes the producers leave at once (the test
// of this path: tests/test_gpu_hmc.py::test_fused_launch_reports_starved_producers).
// The LOCAL launch (hmc_gauss_quad_local_kernel, tuning key "quad_local", the default for D <= 3 with row waves) has no such hand-over:
// its producers are waves of the consumer's own block, behind a barrier.  It takes none of the fields below; "quad_starve" = 1 - a
// producer BLOCK that is never scheduled - selects this cross-block launch, the only one that failure can happen to.
struct QuadFused { uint32_t* flags; int ch; uint32_t target; int nchunks; uint32_t* err; int starve; };
// ROWS (tuning key "quad_rows", default 1): the OUTPUT side of a chain - the proposal's row element q = mu + Tout y, the select of the
// stored element, the row store, the final state, the reject count, the NaN rows of a starved launch - runs on a ROW WAVE of the
// same workgroup (quad_rows_body below); the integrating wave keeps the chain and the accept test and hands each trajectory's
// outcome over through LDS.
//   message   one dword per trajectory and lane: acc ? y : 0xFFFFFFFF.  The sentinel is a NaN pattern, and an accepted y is never
//             NaN (a NaN or infinite y makes lam y^2, hence dH, NaN or -inf, which the compare rejects; a lane with lam = 0 adds a
//             finite eps r to a finite y), so the row wave rebuilds acc and q exactly: the same v_fmac_f32_dpp sequence on the same y.
//   ring      per integrating wave two buffers of one pass each (NU positions x 64 lanes); the slot address is the lane's base
//             register plus the immediate offset of the position in the unrolled pass - no address arithmetic on the hot path.
//   cost      <3, 25>: 67.5 instructions per trajectory on the integrating wave instead of 73.3 (tests/test_quad_rows_resources.py
//             holds it under 68); 0.148 -> 0.139 ms per 1000 trajectories at BASELINE config 2 (profiles/r07a_quad_rows.txt).
//   hand-over one "s_waitcnt lgkmcnt(0) ; s_barrier" per GROUP of trajectories (a pass of NU, a tail pass of NS, a single one) on
//             both roles: the integrator after it filled buffer g % 2, the row wave before it reads it.  The row wave reaches barrier
//             g + 1 only after it has read group g, and the integrator refills buffer g % 2 only after barrier g + 1.  Both roles
//             derive the sequence of groups from the same launch arguments (quad_groups), so every wave of the block - also one
//             whose chains lie past a.C: it integrates the last chain again and stores nothing - reaches every barrier.
// Results are bit-identical to "quad_rows" = 0 (tests/test_gpu_quad_rows.py).
// LOCAL (hmc_gauss_quad_local_kernel below) is ROWS with the record coming from LDS too: the refill between the two butterfly stages
// is a ds_read_b32 at lane base + immediate, the producer waves join the group's barrier, and there is no need_rows.  <3, 25>: 67.6
// instructions per trajectory, no global memory instruction in the pass (tests/test_quad_local_resources.py).
constexpr int quad_fused_ns(int LB, bool FUSED) { return FUSED ? QUAD_FUSED_NS : (LB == 5 ? 4 : (LB == 10 ? 3 : 2)); }
constexpr int quad_nu(int LB, int NS, bool UADDR) { return UADDR ? (LB == 25 ? 8 : 4) * NS : 2 * NS; }
constexpr uint32_t QUAD_ROWS_REJECT = 0xFFFFFFFFu;
// The groups of trajectories of a LOCAL launch (hmc_gauss_quad_local_kernel), in order: f(first trajectory, phase, size, Q2).  The
// integrating wave, its row wave and the producer waves all walk THIS sequence, derived from the launch arguments alone, so every
// wave of a block reaches the same barriers.  It is the fused launch's sequence (the Q2 trajectory alone, passes of NU, passes of
// NS, single ones; per phase) with one short group of NS in front: the integrator starts after one producer sweep, not after a pass.
template <int NS, int NU, typename F> __device__ __forceinline__ void quad_local_groups(const GaussArgs<float>& a, F&& f) {
  const int n_burn = a.samples ? min(max(a.burn - a.traj_offset + 1, 0), a.n_traj) : a.n_traj;
  std::integral_constant<int, 1> one;
  std::false_type plain;
  int t = 0;
  for (int phase = 0; phase < 2; ++phase) {
    const int t_end = phase == 0 ? n_burn : a.n_traj;
    if (phase == 1 && t < t_end && a.traj_offset + t == a.burn + 1) { f(t, phase, one, std::true_type{}); t += 1; }
    if (t == 0 && NS - 1 < t_end) { f(t, phase, std::integral_constant<int, NS>{}, plain); t += NS; }
    while (t + NU - 1 < t_end) { f(t, phase, std::integral_constant<int, NU>{}, plain); t += NU; }
    while (t + NS - 1 < t_end) { f(t, phase, std::integral_constant<int, NS>{}, plain); t += NS; }
    while (t < t_end) { f(t, phase, one, plain); t += 1; }
  }
}
// WIDE (hmc_gauss_quad_wide_kernel below, tuning key "quad_wide") is LOCAL with 16-byte hand-overs: both rings keep their sizes, but
// position p WITHIN ITS GROUP lives at (p >> 2) * 1024 + lane * 16 + (p & 3) * 4 of a buffer (lane: the integrating wave's), so the
// four positions of a block of four are one ds_read_b128 / ds_write_b128 per lane.  The integrating wave reads the records of block
// b + 1 inside the first trajectory of block b into the other half of eight record registers (one wait per block) and writes the
// four messages of a block with the select that completes it (or in the hand-over); the butterfly's wait states that were LDS
// instructions are one "s_nop 1".  The 16-byte accesses are typed LDS accesses the compiler sees: it keeps their wait counts and
// the hazard of a wide store's data registers.  Arithmetic, the sequence of groups (quad_local_groups) and the number and order of
// s_barriers of every role are exactly LOCAL's - only addresses and LDS instructions differ, so there is no new way to hang.
//
// The launch FORMS, by name: what quad_body, quad_rows_body and quad_local_produce are instantiated with (D and LB stay ordinary
// parameters).  Each form is the one above it with one more flag.
struct QuadFormBase { static constexpr bool DIAG = false, FUSED = false, ROWS = false, LOCAL = false, WIDE = false, PROP = false; static constexpr int VAR = 7; };
template <bool DIAG_, int VAR_> struct QuadPlain : QuadFormBase { static constexpr bool DIAG = DIAG_; static constexpr int VAR = VAR_; };      // hmc_gauss_quad_kernel: records from a pre-draw launch
struct QuadFusedForm : QuadFormBase { static constexpr bool FUSED = true; };      // producer blocks behind the consumers' (hmc_gauss_quad_fused_kernel, NI = 0)
struct QuadRowsForm : QuadFusedForm { static constexpr bool ROWS = true; };       // ... the output side on row waves (NI > 0)
struct QuadLocalForm : QuadRowsForm { static constexpr bool LOCAL = true; };      // ... the records from producer waves of the block (hmc_gauss_quad_local_kernel)
struct QuadWideForm : QuadLocalForm { static constexpr bool WIDE = true; };       // ... 16-byte hand-overs (hmc_gauss_quad_wide_kernel, hmc_gauss_quad_lead_kernel)
// PROP (tuning key "quad_prop", default 1): the twin of any form above whose trajectory applies the half kick, the L steps and the
// closing half kick as ONE precomputed linear map  y = a yc + b z ; r = c yc + d z  (quad_prop.hpp: the coefficients are the same
// straight-line arithmetic in float64 on two basis inputs, computed once per launch and lane, in front of the first group) - four
// instructions instead of 2 L + 2, closer to the float64 trajectory than the float32 chain of steps.  Energies, the butterfly, the
// compare, the selects, the message, Q2, burn and the NaN rules are the form's own: a coefficient that overflowed makes y or r
// infinite or NaN, hence dH -inf or NaN, which rejects.  The arithmetic does not depend on the step count at compile time, so a
// twin has no LB instances: it takes the pass shape of LB = 25 (QUAD_PROP_LB) and a look-ahead of four records in every form.
template <typename Base> struct QuadPropOf : Base { static constexpr bool PROP = true; };
constexpr int QUAD_PROP_LB = 25;
template <int D, int LB, typename Form>
__device__ __forceinline__ void quad_body(const GaussArgs<float>& a, const float* __restrict__ eig, const int64_t gt, const QuadFused fz,
                                          uint32_t lds = 0, uint32_t recl = 0) {
  typedef float T;
  constexpr bool DIAG = Form::DIAG, FUSED = Form::FUSED, ROWS = Form::ROWS, LOCAL = Form::LOCAL, WIDE = Form::WIDE;
  constexpr int VAR = Form::VAR;
  constexpr bool PROP = Form::PROP;
  static_assert(!PROP || LB == QUAD_PROP_LB, "a propagator twin has one pass shape");
  constexpr bool UADDR = (VAR & 1) != 0, NOGUARD = (VAR & 2) != 0, TAIL = (VAR & 4) != 0;
  static_assert(!Form::ROWS || (Form::FUSED && UADDR && TAIL && !Form::DIAG), "the row-wave form is an instance of the fused launch");
  static_assert(!Form::LOCAL || (Form::ROWS && D < 4), "the local launch is the row-wave form with one record vector");
  static_assert(!Form::WIDE || (Form::LOCAL && QUAD_FUSED_NS == 4), "the wide hand-over is the local launch's, in blocks of four positions");
  typedef float V4f __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) V4f* lvec_t;
  const bool on = (gt >> 2) < a.C;
  const int64_t c = ROWS ? (on ? gt >> 2 : a.C - 1) : gt >> 2;       // ROWS: every wave stays for the barriers
  const int k = (int)(gt & 3);
  if constexpr (!ROWS) { if (c >= a.C) return; }                     // whole quads leave together
  // FUSED: rows [0, ready) are known complete; the counter of the chunk that starts at row `ready` was requested when the previous
  // chunk was confirmed (pf).  The hot path pays one compare per pass; the poll runs once per chunk, out of the straight line.
  int ready = 0;
  uint32_t pf = 0;
  bool starved = false;
  if constexpr (FUSED && !LOCAL) pf = __hip_atomic_load(fz.flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  auto need_rows = [&](int upto) {              // rows up to `upto` are about to be read (rows >= n_traj are slack: never produced)
    if constexpr (FUSED && !LOCAL) {            // (LOCAL: the block's own producer waves, published by the barrier of the group)
      if (__builtin_expect(upto >= ready, 0)) {
        do {
          const int chn = ready / fz.ch;
          if (chn >= fz.nchunks) { ready = 0x7fffffff; break; }
          uint32_t v = pf;
          // (bounded - ~1 s of polling: producers wait for nothing, so they count as soon as they are scheduled; one that is not
          //  would otherwise hang the queue)
          for (int spin = 0; v < fz.target && spin < (1 << 20); ++spin) {
            __builtin_amdgcn_s_sleep(4);
            v = __hip_atomic_load(fz.flags + chn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          if (__builtin_expect(v < fz.target, 0)) {          // the bound expired: sticky status word, no more waiting, NaN rows at the end
            __hip_atomic_fetch_or(fz.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            starved = true;
            ready = 0x7fffffff;
            break;
          }
          ready += fz.ch;
          pf = chn + 1 < fz.nchunks ? __hip_atomic_load(fz.flags + chn + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        } while (upto >= ready);
        __atomic_signal_fence(__ATOMIC_SEQ_CST);  // the record loads below stay below
      }
    }
  };
  const bool live = k < D;
  const int kk = live ? k : 0;                  // a dummy lane (k >= D) mirrors lane 0 on the output side (same address, same value)
  const T lam = live ? eig[kk] : 0.f;
  const T mu = a.mu[kk];
  T Qrow[D], Qcol[D];                           // Q[k][j] and Q[j][k]
#pragma unroll
  for (int j = 0; j < D; ++j) {
    Qrow[j] = eig[EIG_TOUT(D) + kk * D + j];                  // q_k = mu_k + sum_j Tout[k][j] y_j
    Qcol[j] = live ? eig[EIG_TIN(D) + kk * D + j] : 0.f;     // y_k = sum_i Tin[k][i] (q_i - mu_i)
  }
  // a dummy lane integrates nothing: eps = lam = 0, so its y stays 0, its r stays whatever its record slot held (log u or
  // padding) and its energy difference is exactly 0
  const T eps = live ? a.eps : 0.f, nel = -(eps * lam), hl = 0.5f * eps * lam;
  QuadProp pc{1.f, 0.f, 0.f, 1.f};
  if constexpr (PROP) pc = quad_prop_coeffs(eps, nel, hl, a.L);      // once per launch, while the first records are on their way
  const size_t C = (size_t)a.C;
  auto bc = [&](T v, int j) {                   // lane j of the quad (j compile-time after unrolling)
    return j == 0 ? quad_bcast<0>(v) : j == 1 ? quad_bcast<1>(v) : j == 2 ? quad_bcast<2>(v) : quad_bcast<3>(v);
  };
  auto to_y = [&](const T* __restrict__ q) {    // y_k = sum_i Q[i][k] (q_i - mu_i)
    const T d = live ? q[c * D + kk] - mu : 0.f;
    T y = Qcol[0] * bc(d, 0);
#pragma unroll
    for (int i = 1; i < D; ++i) y = fmaf(Qcol[i], bc(d, i), y);
    return y;
  };
  auto to_q = [&](T y) {                         // q_k = mu_k + sum_j Q[k][j] y_j: v_fmac_f32 with a DPP-broadcast operand
    T q = mu;
    // VALU write of y -> DPP read: 2 wait states (inline asm is not tracked); tied to y so it cannot move ahead of y's producer
    asm volatile("s_nop 1" : "+v"(y));
#pragma unroll
    for (int j = 0; j < D; ++j)
      asm volatile("v_fmac_f32_dpp %0, %1, %2 quad_perm:[%3,%3,%3,%3] row_mask:0xf bank_mask:0xf"
                   : "+v"(q) : "v"(y), "v"(Qrow[j]), "n"(j));
    return q;
  };
  T yc = to_y(a.theta);
  // the row element this lane stores: kept as it was written (a rejected trajectory repeats the previous row bit for bit,
  // the first rows repeat params_init exactly, S:1018) - only an accepted proposal is mapped back, q = mu + Tout y
  T qc = ROWS ? 0.f : a.theta[c * D + kk];        // (ROWS: the row wave's)
  // Energies are carried DOUBLED (2 x potential share = lam y^2, 2 x kinetic share = r^2; the record holds 2 log u): one
  // multiply less per energy, and scaling by two commutes with rounding, so the decisions are those of the plain form.
  T potc = lam * yc * yc;                        // twice this coordinate's share of the potential at the current point
  int32_t accepted = 0;

  // The record pointer is per lane and advances with one 64-bit vector add per trajectory (a scalar base would take an
  // s_add / s_addc pair: at this size a scalar instruction costs what a vector one does).
  constexpr int W = rec_elems<T, D>();
  typedef const __attribute__((address_space(1))) T* grec_t;       // stays a global pointer through the ordering asm below
  grec_t rec = (grec_t)(a.ws_z + (size_t)c * W + k);               // element k of this chain's record (W >= 4 floats)
  const int ushift = D - k;                                        // D == 4: log u sits in the second vector
  const size_t rec_step = C * W;
  // Records are read NS trajectories ahead: a trajectory (~90 ns at L = 5, ~180 ns at L = 25) is shorter than the ~250 ns
  // an HBM load takes to return, and the look-ahead has to cover it.  The workspace carries QUAD_SLOTS rows of slack.
  constexpr int NS = PROP ? QUAD_FUSED_NS : quad_fused_ns(LB, FUSED);     // (FUSED: the records come from memory, not from this XCD's L2; PROP: a trajectory is a fraction of a load's latency)
  static_assert(NS <= QUAD_SLOTS, "workspace slack");
  constexpr int NZ = WIDE ? 8 : NS;                // (WIDE: the block being consumed and the block being read)
  T zs[NZ], lus[NZ];
  T mq[4] = {0.f, 0.f, 0.f, 0.f};                  // WIDE: the messages of the block being completed
  need_rows(NS - 1);
  if constexpr (LOCAL) {
#pragma unroll
    for (int i = 0; i < NZ; ++i) zs[i] = lus[i] = 0.f;      // (begin() below reads the first records of every group)
  } else {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      if (i) rec += rec_step;
      zs[i] = *rec;
      lus[i] = D == 4 ? *(rec + ushift) : 0.f;
    }
  }
  // Every lane stores once per trajectory, unconditionally (uniform vmcnt, see hmc_gauss_small_kernel).
  const uint32_t qoff = (uint32_t)(((size_t)c * D + kk) * sizeof(T));
  typedef __attribute__((address_space(1))) char* gwbytes_t;
  auto put = [&](gwbytes_t row, T v) { *(__attribute__((address_space(1))) T*)(row + qoff) = v; };
  if constexpr (!ROWS) put((gwbytes_t)a.theta, to_q(yc));
  // UADDR: the record of the trajectory at position i of the unrolled loop is recb + roff[i] (recb: the row NS ahead of the
  // pass's first trajectory), its stored row element rowb + soff[i]; both bases are wave-uniform and move once per pass.
  // (the dispatcher bounds C so that the offsets stay below 2^32)
  constexpr int NU = quad_nu(LB, NS, UADDR);       // trajectories per pass of the unrolled loop (the scalar bookkeeping of a pass is shared)
  // ROWS: the message of the trajectory at position i of a group goes to lds + 256 i (64 lanes x 4 bytes); `lds` flips between the two buffers
  const uint32_t lds_both = 2u * lds + (uint32_t)(NU * 256), recl_both = 2u * recl + (uint32_t)(NU * 256);
  T pend_y = 0.f;                                // the last trajectory's proposal and decision: its message is still to be written (D < 4)
  uint64_t pend_mask = 0;
  auto handover = [&](auto G) {                  // after a group of G trajectories
    if constexpr (ROWS) {
      if constexpr (WIDE && decltype(G)::value >= 4) {      // the group's last message completes its last block
        asm volatile("v_cndmask_b32_e64 %0, -1, %1, %2" : "=v"(mq[3]) : "v"(pend_y), "s"(pend_mask));
        *(lvec_t)(uintptr_t)(lds + (uint32_t)((decltype(G)::value / 4 - 1) * 1024)) = V4f{mq[0], mq[1], mq[2], mq[3]};
      } else if constexpr (D < 4) {                          // (WIDE: a group of one is slot 0 of block 0 - the same dword)
        T msg;
        asm volatile("v_cndmask_b32_e64 %0, -1, %1, %2\n\tds_write_b32 %3, %0 offset:%4"
                     : "=&v"(msg) : "v"(pend_y), "s"(pend_mask), "v"(lds), "n"((decltype(G)::value - 1) * 256));
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      lds = lds_both - lds;
      if constexpr (LOCAL) recl = recl_both - recl;
    }
  };
  // LOCAL: the record element of the trajectory at position i of a group is at recl + 256 i (16 chains x 16 bytes: this lane's element
  // of its chain's record is the lane's own dword), in the buffer the producer waves filled during the previous group and the
  // barrier in front of this one published.  A group reads its first NS elements here and, inside trajectory P, the element of
  // trajectory P + NS - never past the group: the other buffer is being written.
  typedef const __attribute__((address_space(3))) T* lrec_t;
  auto begin = [&](auto G) {
    if constexpr (WIDE && decltype(G)::value >= 4) {      // block 0 of the group; block b + 1 is read inside the first trajectory of block b
      const V4f v = *(lvec_t)(uintptr_t)recl;
      zs[0] = v[0]; zs[1] = v[1]; zs[2] = v[2]; zs[3] = v[3];
    } else if constexpr (LOCAL) {                           // (WIDE: a group of one is slot 0 of block 0 - the same dword)
#pragma unroll
      for (int i = 0; i < (decltype(G)::value < NS ? decltype(G)::value : NS); ++i)      // (volatile: four ds_read_b32, not two paired reads - the loop's count is pinned)
        zs[i] = *(const volatile __attribute__((address_space(3))) T*)(uintptr_t)(recl + (uint32_t)i * 256u);
    }
  };
  typedef const __attribute__((address_space(1))) char* gcbytes_t;
  gcbytes_t recb = (gcbytes_t)a.ws_z + (size_t)NS * (rec_step * sizeof(T));
  uint32_t roff[NU], uoff[NU], soff[NU];
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    roff[i] = (uint32_t)((c * W + k) * sizeof(T)) + (uint32_t)i * (uint32_t)(rec_step * sizeof(T));
    uoff[i] = roff[i] + (uint32_t)(ushift * sizeof(T));
    soff[i] = qoff;
  }
  // Two phases, one loop body: trajectories with n <= burn rewrite the chain's slot of `theta` (row step 0), the others
  // walk the sample rows.
  const int n_burn = a.samples ? min(max(a.burn - a.traj_offset + 1, 0), a.n_traj) : a.n_traj;
  int t = 0;
  for (int phase = 0; phase < 2; ++phase) {
    const int t_end = phase == 0 ? n_burn : a.n_traj;
    gwbytes_t row = (gwbytes_t)a.theta;
    size_t row_step = 0;
    if (phase == 1) {
      row = (gwbytes_t)(a.samples + (size_t)max(a.traj_offset + t - a.burn, 1) * C * D);
      row_step = C * D * sizeof(T);
    }
    if constexpr (UADDR) {
#pragma unroll
      for (int i = 0; i < NU; ++i) soff[i] = qoff + (uint32_t)i * (uint32_t)row_step;
    }
    // one trajectory; `slot` holds its record element and is refilled with the one two trajectories ahead (the loop is
    // unrolled by two over the slots, so the newest load is never touched by a register rotation)
    // `q2`: this is trajectory burn+1, the one the reference resets to params_init when it is rejected (S:1016-1018);
    // a separate instance, so that the others carry no check for it.
    auto trajectory = [&](T& slot, T& slot_u, auto q2, auto pos, auto grp) {      // (grp: the size of the trajectory's group, LOCAL reads it)
      if constexpr (!UADDR) rec += rec_step;
      // everything that reads the record first, so that its register is free for the refill
      // ---- gibbs S:185-186 (rotated draws), H_old S:971, half kick S:281
      T y = yc, r, eo, logu;
      {
        const T z = slot;
        if constexpr (ROWS && D < 4) logu = 0.f;      // (broadcast inside the butterfly block below: one of its wait states)
        else
        logu = D == 4 ? slot_u
                      : __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, z), (D < 4 ? D : 0) * 0x55,
                                                                            0xF, 0xF, true));
        eo = fmaf(z, z, potc);
        if constexpr (PROP) { y = fmaf(pc.b, z, pc.a * yc); r = fmaf(pc.d, z, pc.c * yc); }      // the whole trajectory: S:281-302
        else r = fmaf(-hl, yc, z);
      }
      // (the empty asm orders the refill after the record's last use, so the load can target the record's own register;
      //  otherwise the scheduler hoists the load and the back-edge copy of its result waits for it)
      if constexpr (ROWS && D < 4) {
      } else if constexpr (UADDR) {
        if constexpr (PROP) asm volatile("" : "+v"(roff[pos]) : "v"(r), "v"(eo), "v"(logu), "v"(y));
        else asm volatile("" : "+v"(roff[pos]) : "v"(r), "v"(eo), "v"(logu));
        slot = *(grec_t)(recb + roff[pos]);
        if (D == 4) slot_u = *(grec_t)(recb + uoff[pos]);
      } else {
        if constexpr (PROP) asm volatile("" : "+v"(rec) : "v"(r), "v"(eo), "v"(logu), "v"(y));
        else asm volatile("" : "+v"(rec) : "v"(r), "v"(eo), "v"(logu));
        slot = *rec;
        if (D == 4) slot_u = *(rec + ushift);
      }
      if constexpr (PROP) {
      } else if constexpr (LB > 0) {                                                // S:283-298
#pragma unroll
        for (int l = 0; l < LB; ++l) { y = fmaf(eps, r, y); r = fmaf(nel, y, r); }
      } else {
        repeat_steps(a.L, [&]() { y = fmaf(eps, r, y); r = fmaf(nel, y, r); });
      }
      if constexpr (!PROP) r = fmaf(hl, y, r);                                      // S:302
      // ---- H_new S:995 and the MH test S:1000-1004
      const T pot1 = lam * y * y;
      const T en = fmaf(r, r, pot1);
      // the proposal's row element q_k = mu_k + sum_j Tout[k][j] y_j: v_fmac_f32 with a DPP-broadcast operand.  Ordered after
      // `en` (dummy operand): the instructions since the last write of y are the wait states its DPP read needs.
      T qp, dH;
      static_assert(D >= 1 && D <= 4, "quad kernel");
#define HTA_QF(J, OP) "\n\tv_fmac_f32_dpp %0, %1, %" #OP " quad_perm:[" #J "," #J "," #J "," #J "] row_mask:0xf bank_mask:0xf"
      if constexpr (TAIL) {
        // One block for the row element AND the quad butterfly of the energy difference, interleaved so that every DPP read of
        // a freshly written register has its two wait states from useful instructions (the compiler does not look into inline
        // assembly and pads its own DPP pairs with s_nop: one issue slot per trajectory):
        //   d = eo - en (compiler) | mov qp, mu | qp += Q[k][0] y_0 | d += d[lane^1] | qp += Q[k][1] y_1 | ... | d += d[lane^2]
#define HTA_QG(J, OP) "\n\tv_fmac_f32_dpp %0, %2, %" #OP " quad_perm:[" #J "," #J "," #J "," #J "] row_mask:0xf bank_mask:0xf"
#define HTA_B1 "\n\tv_add_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1"
#define HTA_B2 "\n\tv_add_f32_dpp %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1"
        dH = eo - en;
        if constexpr (ROWS && D < 4) {
          // The row element is the row wave's.  The two wait states in front of each stage of the butterfly are useful instructions:
          //   d = eo - en (compiler) | select of the PREVIOUS trajectory's message | log u broadcast | d += d[lane^1] | LDS write of that
          //   message | record refill (compiler; volatile asm on both sides keeps it there) | d += d[lane^2]
          // - the message of a trajectory is selected and written one trajectory late (the last one of a group: flush, before the
          // hand-over), so the integrating wave spends no s_nop on the butterfly; the first trajectory of a group has no message to
          // carry and pads with two.
          qp = 0.f;
          constexpr int P = decltype(pos)::value;
          if constexpr (WIDE) {
            // The same blocks with the LDS instructions once per block of four positions: the select of trajectory P - 1's message
            // targets mq[(P - 1) % 4]; the select of a block's last message (P % 4 == 0, P > 0) is followed by the 16-byte write of
            // the block, and the first trajectory of a block reads the records of the next block of the group into the other half
            // of zs.  A trajectory that issues no LDS instruction (three of four) has its tail in ONE asm block, the second stage's
            // two wait states being one "s_nop 1" (the compiler pads between two blocks).  The first trajectory of a block keeps
            // the local launch's form: the typed LDS accesses (or an "s_nop 0") sit between two volatile asm blocks and are the
            // wait states of the second stage; tests/test_quad_wide_resources.py checks in the built code that every second
            // stage has its two wait states.
            constexpr int Gs = decltype(grp)::value;
            constexpr bool rd = P % 4 == 0 && P + 4 < Gs, wr = P % 4 == 0 && P > 0;
#define HTA_WB1 "\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1"
#define HTA_WT2 "\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_cmp_ge_f32_e64 %3, %0, %1" \
                "\n\tv_cndmask_b32_e64 %2, %2, %5, %3"
            if constexpr (!rd && !wr && P > 0) {
              asm volatile("v_cndmask_b32_e64 %4, -1, %7, %3\n\tv_mov_b32_dpp %1, %6 quad_perm:[%8,%8,%8,%8] row_mask:0xf bank_mask:0xf bound_ctrl:1"
                           HTA_WB1 "\n\ts_nop 1" HTA_WT2
                           : "+v"(dH), "=&v"(logu), "+v"(yc), "+s"(pend_mask), "=&v"(mq[(P + 3) % 4])
                           : "v"(y), "v"(slot), "v"(pend_y), "n"(D));
            } else if constexpr (!rd && !wr) {
              T none;
              asm volatile("v_mov_b32_dpp %1, %6 quad_perm:[%8,%8,%8,%8] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 0"
                           HTA_WB1 "\n\ts_nop 1" HTA_WT2
                           : "+v"(dH), "=&v"(logu), "+v"(yc), "+s"(pend_mask), "=&v"(none)
                           : "v"(y), "v"(slot), "v"(pend_y), "n"(D));
            } else {
              if constexpr (wr) {
                asm volatile("v_cndmask_b32_e64 %2, -1, %4, %5\n\tv_mov_b32_dpp %1, %3 quad_perm:[%6,%6,%6,%6] row_mask:0xf bank_mask:0xf bound_ctrl:1"
                             HTA_WB1
                             : "+v"(dH), "=&v"(logu), "=&v"(mq[3]) : "v"(slot), "v"(pend_y), "s"(pend_mask), "n"(D));
                *(lvec_t)(uintptr_t)(lds + (uint32_t)((P / 4 - 1) * 1024)) = V4f{mq[0], mq[1], mq[2], mq[3]};
              } else {
                asm volatile("v_mov_b32_dpp %1, %2 quad_perm:[%3,%3,%3,%3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 0" HTA_WB1 "\n\ts_nop 0"
                             : "+v"(dH), "=&v"(logu) : "v"(slot), "n"(D));
              }
              if constexpr (rd) {
                constexpr int nb = P / 4 + 1;
                const V4f v = *(lvec_t)(uintptr_t)(recl + (uint32_t)(nb * 1024));
                zs[(nb % 2) * 4] = v[0]; zs[(nb % 2) * 4 + 1] = v[1]; zs[(nb % 2) * 4 + 2] = v[2]; zs[(nb % 2) * 4 + 3] = v[3];
              } else asm volatile("s_nop 0");
              asm volatile("v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_cmp_ge_f32_e64 %2, %0, %3\n\t"
                           "v_cndmask_b32_e64 %1, %1, %4, %2"
                           : "+v"(dH), "+v"(yc), "=&s"(pend_mask) : "v"(logu), "v"(y));
            }
            // (the select of potc is a block of its own, free to sink to potc's next use; the compiler pads one wait state between
            //  the block above and the next trajectory's first FMA, which reads yc - where the local launch has its s_waitcnt)
            asm volatile("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(potc) : "v"(pot1), "s"(pend_mask));
#undef HTA_WB1
#undef HTA_WT2
            pend_y = y;
          } else {
          if constexpr (P > 0) {
            T msg;
            asm volatile("v_cndmask_b32_e64 %2, -1, %4, %5\n\tv_mov_b32_dpp %1, %3 quad_perm:[%8,%8,%8,%8] row_mask:0xf bank_mask:0xf bound_ctrl:1"
                         "\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1"
                         "\n\tds_write_b32 %6, %2 offset:%7"
                         : "+v"(dH), "=&v"(logu), "=&v"(msg)
                         : "v"(slot), "v"(pend_y), "s"(pend_mask), "v"(lds), "n"((P - 1) * 256), "n"(D));
          } else {
            asm volatile("v_mov_b32_dpp %1, %2 quad_perm:[%3,%3,%3,%3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 0" "\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1" "\n\ts_nop 0"
                         : "+v"(dH), "=&v"(logu) : "v"(slot), "n"(D));
          }
          if constexpr (LOCAL) {
            // the refill is an LDS read the compiler sees and waits for (the message writes it does not see only make its count
            // stricter: LDS returns in order); the last NS trajectories of a group have nothing to read and pad the wait state
            if constexpr (P + NS < decltype(grp)::value) slot = *(lrec_t)(uintptr_t)(recl + (uint32_t)(P + NS) * 256u);
            else asm volatile("s_nop 0");
          } else {
          asm volatile("" : "+v"(roff[pos]));            // keeps the zero-extension next to its use: base + 32-bit offset addressing
          slot = *(grec_t)(recb + roff[pos]);
          }
          // second stage, the compare and the selects of yc and potc in one block (the compiler pads a wait state between two blocks)
          asm volatile("v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\tv_cmp_ge_f32_e64 %3, %0, %4\n\t"
                       "v_cndmask_b32_e64 %1, %1, %5, %3\n\tv_cndmask_b32_e64 %2, %2, %6, %3"
                       : "+v"(dH), "+v"(yc), "+v"(potc), "=&s"(pend_mask) : "v"(logu), "v"(y), "v"(pot1));
          pend_y = y;                                    // its message: inside the next trajectory's block, or by the hand-over
          }
        }
        else if constexpr (ROWS) { qp = 0.f; dH = quad_sum(dH); }      // (D = 4: log u is a second record element; the compiler pads the DPP wait states)
        else if constexpr (D == 1)
          asm volatile("v_mov_b32 %0, %3" HTA_QG(0, 4) HTA_B1 "\n\ts_nop 1" HTA_B2
                       : "=&v"(qp), "+v"(dH) : "v"(y), "v"(mu), "v"(Qrow[0]));
        else if constexpr (D == 2)
          asm volatile("v_mov_b32 %0, %3" HTA_QG(0, 4) HTA_B1 HTA_QG(1, 5) "\n\ts_nop 0" HTA_B2
                       : "=&v"(qp), "+v"(dH) : "v"(y), "v"(mu), "v"(Qrow[0]), "v"(Qrow[D > 1 ? 1 : 0]));
        else if constexpr (D == 3)
          asm volatile("v_mov_b32 %0, %3" HTA_QG(0, 4) HTA_B1 HTA_QG(1, 5) HTA_QG(2, 6) HTA_B2
                       : "=&v"(qp), "+v"(dH) : "v"(y), "v"(mu), "v"(Qrow[0]), "v"(Qrow[D > 1 ? 1 : 0]), "v"(Qrow[D > 2 ? 2 : 0]));
        else
          asm volatile("v_mov_b32 %0, %3" HTA_QG(0, 4) HTA_B1 HTA_QG(1, 5) HTA_QG(2, 6) HTA_B2 HTA_QG(3, 7)
                       : "=&v"(qp), "+v"(dH) : "v"(y), "v"(mu), "v"(Qrow[0]), "v"(Qrow[D > 1 ? 1 : 0]), "v"(Qrow[D > 2 ? 2 : 0]),
                         "v"(Qrow[D > 3 ? 3 : 0]));
#undef HTA_QG
#undef HTA_B1
#undef HTA_B2
      } else {
        if constexpr (D == 1)
          asm volatile("v_mov_b32 %0, %2" HTA_QF(0, 4) : "=&v"(qp) : "v"(y), "v"(mu), "v"(en), "v"(Qrow[0]));
        else if constexpr (D == 2)
          asm volatile("v_mov_b32 %0, %2" HTA_QF(0, 4) HTA_QF(1, 5)
                       : "=&v"(qp) : "v"(y), "v"(mu), "v"(en), "v"(Qrow[0]), "v"(Qrow[D > 1 ? 1 : 0]));
        else if constexpr (D == 3)
          asm volatile("v_mov_b32 %0, %2" HTA_QF(0, 4) HTA_QF(1, 5) HTA_QF(2, 6)
                       : "=&v"(qp) : "v"(y), "v"(mu), "v"(en), "v"(Qrow[0]), "v"(Qrow[D > 1 ? 1 : 0]), "v"(Qrow[D > 2 ? 2 : 0]));
        else
          asm volatile("v_mov_b32 %0, %2" HTA_QF(0, 4) HTA_QF(1, 5) HTA_QF(2, 6) HTA_QF(3, 7)
                       : "=&v"(qp) : "v"(y), "v"(mu), "v"(en), "v"(Qrow[0]), "v"(Qrow[D > 1 ? 1 : 0]), "v"(Qrow[D > 2 ? 2 : 0]),
                         "v"(Qrow[D > 3 ? 3 : 0]));
        dH = quad_sum(eo - en);                                                       // 2 (h_old - h_new)
      }
#undef HTA_QF
      // the decision as a lane mask (v_cmp into an SGPR pair), consumed by a carry-in add and two selects
      // rho = min(0, dH) >= log u  <=>  dH >= log u, because log u <= 0 (S:1000-1004).  A non-finite dH must reject:
      // fma(dH, 0, dH) is dH when dH is finite and NaN otherwise (inf * 0), and NaN >= x is false - one compare in all.
      const uint64_t accmask = (ROWS && D < 4) ? pend_mask : __builtin_amdgcn_fcmpf(NOGUARD ? dH : __builtin_fmaf(dH, 0.0f, dH), logu, 3 /* oge */);
      if constexpr (ROWS) {
        // yc, potc <- accepted point; the message acc ? y : sentinel (-1 is an inline constant) into this position's slot of the ring.
        // The accepted count is the row wave's as well.  (D < 4: all of it happened in the butterfly blocks above.)
        if constexpr (D == 4) {
          T msg;
          asm volatile("v_cndmask_b32_e64 %0, %0, %3, %5\n\tv_cndmask_b32_e64 %1, %1, %4, %5\n\tv_cndmask_b32_e64 %2, -1, %3, %5\n\t"
                       "ds_write_b32 %6, %2 offset:%7"
                       : "+v"(yc), "+v"(potc), "=&v"(msg)
                       : "v"(y), "v"(pot1), "s"(accmask), "v"(lds), "n"(decltype(pos)::value * 256));
        }
        if constexpr (decltype(q2)::value) {
          if (!((accmask >> (threadIdx.x & 63)) & 1)) { yc = to_y(a.theta_init); potc = lam * yc * yc; }      // Q2: back to params_init itself
        }
      } else if constexpr (!decltype(q2)::value) {
        // accepted += acc; yc, potc, qc <- accepted point: a carry-in add and three selects on the accept mask
        uint64_t carry_out;
        asm volatile("v_addc_co_u32_e64 %0, %4, 0, %0, %5\n\tv_cndmask_b32_e64 %1, %1, %6, %5\n\tv_cndmask_b32_e64 %2, %2, %7, %5\n\t"
                     "v_cndmask_b32_e64 %3, %3, %8, %5"
                     : "+v"(accepted), "+v"(yc), "+v"(potc), "+v"(qc), "=&s"(carry_out)
                     : "s"(accmask), "v"(y), "v"(pot1), "v"(qp));
      } else {
        uint64_t carry_out;
        asm("v_addc_co_u32_e64 %0, %1, 0, %0, %2" : "+v"(accepted), "=s"(carry_out) : "s"(accmask));
        asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(yc) : "v"(y), "s"(accmask));
        asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(potc) : "v"(pot1), "s"(accmask));
        asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(qc) : "v"(qp), "s"(accmask));
        if (!((accmask >> (threadIdx.x & 63)) & 1)) {        // Q2: back to params_init itself
          yc = to_y(a.theta_init); potc = lam * yc * yc; qc = a.theta_init[c * D + kk];
        }
      }
      if constexpr (ROWS) {
      } else if constexpr (UADDR) {
        asm volatile("" : "+v"(soff[pos]));            // keeps the zero-extension next to its use: base + 32-bit offset addressing
        *(__attribute__((address_space(1))) T*)(row + soff[pos]) = qc;
      } else {
        put(row, qc);
        row += row_step;
      }
      if (DIAG) {
        const bool acc = (accmask >> (threadIdx.x & 63)) & 1;
        // (a dummy lane's eo and en are both the square of its record slot - 2 log u on lane D: they cancel in dH, not in the energies)
        const T ho = 0.5f * quad_sum(live ? eo : 0.f) - a.log_norm, hn = 0.5f * quad_sum(live ? en : 0.f) - a.log_norm;
        if (k == 0) {
          if (a.H_old) a.H_old[(size_t)t * C + c] = ho;
          if (a.H_new) a.H_new[(size_t)t * C + c] = hn;
          if (a.accept) a.accept[(size_t)t * C + c] = acc ? 1 : 0;
        }
      }
      ++t;
    };
    std::false_type plain;
    std::integral_constant<int, 0> first;
    auto rotate = [&]() {                       // slot 0 was consumed and refilled with the newest row: it becomes the last
      const T z = zs[0], u = lus[0];
#pragma unroll
      for (int i = 0; i + 1 < NS; ++i) { zs[i] = zs[i + 1]; lus[i] = lus[i + 1]; }
      zs[NS - 1] = z; lus[NS - 1] = u;
    };
    if constexpr (LOCAL) {
      // the groups of the launch as every role of the block walks them (quad_local_groups); the barrier in front of the first
      // group publishes its records
      if (phase == 0) {
        asm volatile("s_barrier" ::: "memory");
        quad_local_groups<NS, NU>(a, [&](int, int, auto G, auto q2) {
          begin(G);
          quad_static_for<0, decltype(G)::value>([&](auto I) { trajectory(zs[I % NZ], lus[I % NZ], q2, I, G); });
          handover(G);
        });
      }
    } else if constexpr (UADDR) {
      // the same schedule with the bases moved once per group of trajectories
      auto moved = [&](int g) { recb += (size_t)g * (rec_step * sizeof(T)); row += (size_t)g * row_step; };
      // (FUSED: a pass of G trajectories starting at t prefetches the rows up to t + G - 1 + NS)
      if (phase == 1 && t < t_end && a.traj_offset + t == a.burn + 1) {
        need_rows(t + NS);
        trajectory(zs[0], lus[0], std::true_type{}, first, first);
        moved(1);
        rotate();
        handover(std::integral_constant<int, 1>{});
      }
      while (t + NU - 1 < t_end) {
        need_rows(t + NU - 1 + NS);
        quad_static_for<0, NU>([&](auto I) { trajectory(zs[I % NS], lus[I % NS], plain, I, first); });
        moved(NU);
        handover(std::integral_constant<int, NU>{});
      }
      while (t + NS - 1 < t_end) {
        need_rows(t + NS - 1 + NS);
        quad_static_for<0, NS>([&](auto I) { trajectory(zs[I], lus[I], plain, I, first); });
        moved(NS);
        handover(std::integral_constant<int, NS>{});
      }
      while (t < t_end) { need_rows(t + NS); trajectory(zs[0], lus[0], plain, first, first); moved(1); rotate(); handover(std::integral_constant<int, 1>{}); }
    } else {
      if (phase == 1 && t < t_end && a.traj_offset + t == a.burn + 1) {              // the Q2 trajectory opens the stored phase
        trajectory(zs[0], lus[0], std::true_type{}, first, first);
        rotate();
      }
      while (t + 2 * NS - 1 < t_end) {            // unrolled over the slots (twice): no register rotation on the hot path
#pragma unroll
        for (int i = 0; i < 2 * NS; ++i) trajectory(zs[i % NS], lus[i % NS], plain, first, first);
      }
      if (t + NS - 1 < t_end) {
#pragma unroll
        for (int i = 0; i < NS; ++i) trajectory(zs[i], lus[i], plain, first, first);
      }
      while (t < t_end) { trajectory(zs[0], lus[0], plain, first, first); rotate(); }
    }
  }
  if constexpr (ROWS) {                           // one more group: whether this wave's hand-over from the producers failed
    asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" :: "v"(lds), "v"(starved ? 1u : 0u) : "memory");
    return;
  }
  if constexpr (FUSED) {
    if (__builtin_expect(starved, 0)) {           // see QuadFused: the rows of this launch and the chain state become NaN
      qc = __builtin_nanf("");
      if (a.samples) {
        const size_t r0 = (size_t)max(a.traj_offset + n_burn - a.burn, 1);
        for (int tt = n_burn; tt < a.n_traj; ++tt) put((gwbytes_t)(a.samples + (r0 + (size_t)(tt - n_burn)) * C * D), qc);
      }
    }
  }
  put((gwbytes_t)a.theta, qc);
  if (a.reject_count && k == 0) a.reject_count[c] += a.n_traj - accepted;
}

// The row wave of an integrating wave (ROWS above): same lane, same chain, same coordinate.  It walks the groups of trajectories in
// the integrator's order, one barrier in front of each, and owns the output side.  In the burn-in phase it stores no row (the
// one-launch form rewrites the chain's slot of `theta` every trajectory; nobody reads those within the launch): only the final state.
// WT (tuning key "quad_rows_wt", the local and wide launches): the sample row element is stored WRITE-THROUGH at agent scope (a relaxed
// atomic store: global_store_dword ... sc1, a store the compiler tracks), so a launch's 12 MB of rows leave the XCD's L2 while the
// launch runs, not in the write-back of dirty lines behind its last wave (profiles/r15a_quad_lead.txt).  Same value, same address;
// the final state, the reject count and a starved launch's NaN rows stay plain stores.
template <int D, int LB, typename Form>
__device__ __forceinline__ void quad_rows_body(const GaussArgs<float>& a, const float* __restrict__ eig, const int64_t gt, uint32_t lds,
                                               const bool wt = false) {
  typedef float T;
  static_assert(Form::ROWS, "the row wave of a form without row waves");
  constexpr bool LOCAL = Form::LOCAL, WIDE = Form::WIDE;
  constexpr int NS = quad_fused_ns(LB, true), NU = quad_nu(LB, NS, true);
  const bool on = (gt >> 2) < a.C;
  const int64_t c = on ? gt >> 2 : a.C - 1;
  const int k = (int)(gt & 3);
  const int kk = k < D ? k : 0;                 // a dummy lane mirrors lane 0 (same address, same value)
  const T mu = a.mu[kk];
  T Qrow[D];
#pragma unroll
  for (int j = 0; j < D; ++j) Qrow[j] = eig[EIG_TOUT(D) + kk * D + j];
  auto to_q = [&](T y) {                         // quad_body's: the same instructions in the same order
    T q = mu;
    asm volatile("s_nop 1" : "+v"(y));
#pragma unroll
    for (int j = 0; j < D; ++j)
      asm volatile("v_fmac_f32_dpp %0, %1, %2 quad_perm:[%3,%3,%3,%3] row_mask:0xf bank_mask:0xf"
                   : "+v"(q) : "v"(y), "v"(Qrow[j]), "n"(j));
    return q;
  };
  const size_t C = (size_t)a.C;
  const size_t el = (size_t)c * D + kk;
  T qc = a.theta[el];
  int32_t accepted = 0;
  const uint32_t lds_both = 2u * lds + (uint32_t)(NU * 256);
  const int n_burn = a.samples ? min(max(a.burn - a.traj_offset + 1, 0), a.n_traj) : a.n_traj;
  T* row = nullptr;
  auto take = [&](T m, bool q2) {               // one trajectory's message
    const bool acc = __builtin_bit_cast(uint32_t, m) != QUAD_ROWS_REJECT;
    const T q = to_q(m);                         // (every lane: the DPP operands come from the quad's other lanes)
    qc = acc ? q : qc;
    accepted += acc ? 1 : 0;
    if (q2 && !acc) qc = a.theta_init[el];       // Q2: back to params_init itself
    if (row) {
      if (on) {
        if (wt) __hip_atomic_store(row + el, qc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else row[el] = qc;
      }
      row += C * D;
    }
  };
  // PROP forms: four trajectories' messages at once, the way of a whole group decided OUTSIDE (STORE: the stored phase; WT):
  // straight-line code, one exec-mask bracket per four stores.  A propagated trajectory is ~20 instructions on the integrating wave,
  // and take()'s three branches per trajectory (no row yet? chain past a.C? write-through?) made this wave the slower one
  // (profiles/r16a_quad_prop.txt).  Same values, same addresses.  The step-by-step forms keep take(): their code is untouched.
  auto take4 = [&](T m0, T m1, T m2, T m3, auto STORE, auto WT) {
    const T m[4] = {m0, m1, m2, m3};
    // to_q of the four, column by column: per element the same v_fmac_f32_dpp sequence on the same operands (the same bits), the
    // four chains interleaved - the messages come out of LDS, no DPP read follows a VALU write of its source, no wait state is due
    T qs[4];
    asm volatile("v_mov_b32 %0, %4\n\tv_mov_b32 %1, %4\n\tv_mov_b32 %2, %4\n\tv_mov_b32 %3, %4"
                 : "=&v"(qs[0]), "=&v"(qs[1]), "=&v"(qs[2]), "=&v"(qs[3]) : "v"(mu));
#pragma unroll
    for (int jc = 0; jc < D; ++jc)
      asm volatile("v_fmac_f32_dpp %0, %4, %8 quad_perm:[%9,%9,%9,%9] row_mask:0xf bank_mask:0xf\n\t"
                   "v_fmac_f32_dpp %1, %5, %8 quad_perm:[%9,%9,%9,%9] row_mask:0xf bank_mask:0xf\n\t"
                   "v_fmac_f32_dpp %2, %6, %8 quad_perm:[%9,%9,%9,%9] row_mask:0xf bank_mask:0xf\n\t"
                   "v_fmac_f32_dpp %3, %7, %8 quad_perm:[%9,%9,%9,%9] row_mask:0xf bank_mask:0xf"
                   : "+v"(qs[0]), "+v"(qs[1]), "+v"(qs[2]), "+v"(qs[3])
                   : "v"(m[0]), "v"(m[1]), "v"(m[2]), "v"(m[3]), "v"(Qrow[jc]), "n"(jc));
    T v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool acc = __builtin_bit_cast(uint32_t, m[j]) != QUAD_ROWS_REJECT;
      const T q = qs[j];
      qc = acc ? q : qc;
      v[j] = qc;
      accepted += acc ? 1 : 0;
    }
    if constexpr (decltype(STORE)::value) {
      if (on) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if constexpr (decltype(WT)::value) __hip_atomic_store(row + el + (size_t)j * C * D, v[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          else row[el + (size_t)j * C * D] = v[j];
        }
      }
      row += 4 * C * D;
    }
  };
  auto group = [&](auto G, bool q2) {
    asm volatile("s_barrier" ::: "memory");      // the integrator has filled this buffer
    constexpr int g = decltype(G)::value;
    if constexpr (!Form::PROP && WIDE && g % 4 == 0) {           // one 16-byte read per block of four positions (quad_body: WIDE)
      for (int i = 0; i < g; i += 4) {
        typedef float V4f __attribute__((ext_vector_type(4)));
        V4f m;
        asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(m) : "v"(lds + (uint32_t)i * 256u) : "memory");
        take(m[0], false); take(m[1], false); take(m[2], false); take(m[3], false);
      }
    } else if constexpr (!Form::PROP && g % 4 == 0) {
      for (int i = 0; i < g; i += 4) {
        T m0, m1, m2, m3;
        asm volatile("ds_read_b32 %0, %4\n\tds_read_b32 %1, %4 offset:256\n\tds_read_b32 %2, %4 offset:512\n\tds_read_b32 %3, %4 offset:768\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(m0), "=&v"(m1), "=&v"(m2), "=&v"(m3) : "v"(lds + (uint32_t)i * 256u) : "memory");
        take(m0, false); take(m1, false); take(m2, false); take(m3, false);
      }
    } else if constexpr (g % 4 == 0) {                            // PROP: the blocks below
      auto blocks = [&](auto STORE, auto WT) {
        typedef float V4f __attribute__((ext_vector_type(4)));
        typedef const __attribute__((address_space(3))) V4f* lvec_t;
        V4f mw = {0.f, 0.f, 0.f, 0.f};
        if constexpr (WIDE) mw = *(lvec_t)(uintptr_t)lds;      // (typed LDS reads: the compiler keeps their wait counts; the barrier's clobber keeps them behind it)
        for (int i = 0; i < g; i += 4) {
          if constexpr (WIDE) {                   // one 16-byte read per block of four positions (quad_body: WIDE), the next block's
            const V4f m = mw;                     // issued before this block's work: its LDS round trip hides behind four trajectories
            if (i + 4 < g) mw = *(lvec_t)(uintptr_t)(lds + (uint32_t)(i + 4) * 256u);
            take4(m[0], m[1], m[2], m[3], STORE, WT);
          } else {
            T m0, m1, m2, m3;
            asm volatile("ds_read_b32 %0, %4\n\tds_read_b32 %1, %4 offset:256\n\tds_read_b32 %2, %4 offset:512\n\tds_read_b32 %3, %4 offset:768\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         : "=&v"(m0), "=&v"(m1), "=&v"(m2), "=&v"(m3) : "v"(lds + (uint32_t)i * 256u) : "memory");
            take4(m0, m1, m2, m3, STORE, WT);
          }
        }
      };
      if (!row) blocks(std::false_type{}, std::false_type{});
      else if (wt) blocks(std::true_type{}, std::true_type{});
      else blocks(std::true_type{}, std::false_type{});
    } else {
      for (int i = 0; i < g; ++i) {
        T m;
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(m) : "v"(lds + (uint32_t)i * 256u) : "memory");
        take(m, q2);
      }
    }
    lds = lds_both - lds;
  };
  std::integral_constant<int, 1> one;
  int t = 0;
  if constexpr (LOCAL) {                          // the local launch's sequence (its first barrier publishes records: not this wave's business)
    asm volatile("s_barrier" ::: "memory");
    quad_local_groups<NS, NU>(a, [&](int t0, int phase, auto G, auto q2) {
      if (phase == 1 && !row) row = a.samples + (size_t)max(a.traj_offset + t0 - a.burn, 1) * C * D;      // (the stored phase is empty without a.samples)
      group(G, decltype(q2)::value);
    });
  } else
  for (int phase = 0; phase < 2; ++phase) {
    const int t_end = phase == 0 ? n_burn : a.n_traj;
    if (phase == 1) {
      row = a.samples ? a.samples + (size_t)max(a.traj_offset + t - a.burn, 1) * C * D : nullptr;
      if (t < t_end && a.traj_offset + t == a.burn + 1) { group(one, true); t += 1; }
    }
    while (t + NU - 1 < t_end) { group(std::integral_constant<int, NU>{}, false); t += NU; }
    while (t + NS - 1 < t_end) { group(std::integral_constant<int, NS>{}, false); t += NS; }
    while (t < t_end) { group(one, false); t += 1; }
  }
  uint32_t starved;
  asm volatile("s_barrier\n\tds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(starved) : "v"(lds) : "memory");
  if (__builtin_expect(starved != 0u, 0)) {     // see QuadFused: the rows of this launch and the chain state become NaN
    qc = __builtin_nanf("");
    if (a.samples && on) {
      const size_t r0 = (size_t)max(a.traj_offset + n_burn - a.burn, 1);
      for (int tt = n_burn; tt < a.n_traj; ++tt) a.samples[(r0 + (size_t)(tt - n_burn)) * C * D + el] = qc;
    }
  }
  if (on) {
    a.theta[el] = qc;
    if (a.reject_count && k == 0) a.reject_count[c] += a.n_traj - accepted;
  }
}

template <int D, bool DIAG, int LB, int VAR = 0>
__global__ __launch_bounds__(64) void hmc_gauss_quad_kernel(GaussArgs<float> a, const float* __restrict__ eig) {
  quad_body<D, LB, QuadPlain<DIAG, VAR>>(a, eig, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, QuadFused{nullptr, 1, 0u, 0, nullptr, 0});
}
// its propagator twin (quad_body: PROP): any L, the DIAG instance included
template <int D, bool DIAG, int VAR = 0>
__global__ __launch_bounds__(64) void hmc_gauss_quad_prop_kernel(GaussArgs<float> a, const float* __restrict__ eig) {
  quad_body<D, QUAD_PROP_LB, QuadPropOf<QuadPlain<DIAG, VAR>>>(a, eig, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, QuadFused{nullptr, 1, 0u, 0, nullptr, 0});
}

// one record (csrc: rng_fill_small_kernel's body): the draws of trajectory n of global chain `chain`, rotated into the eigenbasis, and
// 2 log u in element D.  The ONE body of the record's arithmetic: the cross-block producers and the local launch's producer waves
// both call it, so their records are the same bits.
template <int D>
__device__ __forceinline__ void quad_make_record(uint64_t seed, uint64_t chain, uint32_t n, const float* __restrict__ eig,
                                                 float (&rec)[rec_elems<float, D>()]) {
  typedef float T;
  constexpr int W = rec_elems<T, D>();
  T z[D], lu;
  draw_inline<T, D>(seed, chain, n, z, lu);
#pragma unroll
  for (int i = 0; i < W; ++i) rec[i] = 0;
#pragma unroll
  for (int kk = 0; kk < D; ++kk) {
    T acc = eig[EIG_QT(D) + kk * D + 0] * z[0];
#pragma unroll
    for (int i = 1; i < D; ++i) acc = fma(eig[EIG_QT(D) + kk * D + i], z[i], acc);
    rec[kk] = acc;
  }
  rec[D] = 2.0f * lu;
}
template <int D>
__device__ __forceinline__ void quad_fill_record(float* __restrict__ ws, int64_t idx, int64_t C, int traj_offset, uint64_t seed,
                                                 uint64_t chain_offset, const float* __restrict__ eig) {
  typedef float T;
  constexpr int W = rec_elems<T, D>();
  const int64_t t = idx / C, c = idx - t * C;
  T rec[W];
  quad_make_record<D>(seed, chain_offset + (uint64_t)c, (uint32_t)(traj_offset + (int)t), eig, rec);
  // write-through stores at agent scope (sc1): the record is in memory, visible to the consumers' XCDs, once the store is
  // acknowledged - no L2 write-back per producer block (a buffer_wbl2 per 64 records made the producers 40x slower)
  // (one 16-byte store with the agent-scope bit: four dword stores quadrupled the write transactions)
  typedef float V4f __attribute__((ext_vector_type(4)));
  static_assert(W % 4 == 0, "records are whole 16-byte words");
#pragma unroll
  for (int i = 0; i < W / 4; ++i) {
    const V4f v = {rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3]};
    const __attribute__((address_space(1))) V4f* dst = (const __attribute__((address_space(1))) V4f*)(ws + idx * W + 4 * i);
    // (s_nop: a store wider than 8 bytes reads its data registers after issue; the compiler pads that hazard for stores it
    //  knows, not for inline assembly - without it the next VALU write into v's registers corrupted the record: D = 4 caught it)
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 2" :: "v"(dst), "v"(v) : "memory");
  }
}

// consumers (blocks [0, nc): the quad kernel's body) and producers (the blocks behind them, chunk-major: block b writes the
// 64-record slice b % spc of chunk b / spc) in ONE launch.  `done` counts the consumer blocks that finished: the last one
// zeroes the counters for the next launch (no memset node, nothing the host has to track: the launch stays graph-capturable).
constexpr int QUAD_FUSED_NT = 256;         // four waves per block: a producer block counts itself ONCE per chunk (the counter of a chunk
                                           // is one address: its atomic adds serialise - 512 one-wave producers were 3x slower than 128)
// NI (tuning key "quad_rows"): 0 = every consumer wave integrates and stores its rows itself (QUAD_FUSED_NT threads); NI > 0 = a block
// of 2 NI waves, waves [0, NI) integrate, wave NI + w is the row wave of wave w (quad_body: ROWS).  A producer block writes the same
// 256-record slices whatever the block size, so the records, the chunk counters and their target do not depend on NI.
constexpr int QUAD_ROWS_NI = 2;            // with two pairs per block the integrating waves and the row waves sit on different SIMDs of the
                                           // CU (waves of a workgroup are dealt out round robin) and the block size is the producers' own
constexpr int quad_fused_threads(int NI) { return NI > 0 ? 128 * NI : QUAD_FUSED_NT; }
template <int D, int LB, int NI, bool PROP>
__device__ __forceinline__ void quad_fused_block(const GaussArgs<float>& a, const float* __restrict__ eig, const QuadFused& fz, int nc, int spc, uint32_t* done) {
  constexpr int NT = quad_fused_threads(NI);
  typedef std::conditional_t<PROP, QuadPropOf<QuadRowsForm>, QuadRowsForm> RowsForm;
  typedef std::conditional_t<PROP, QuadPropOf<QuadFusedForm>, QuadFusedForm> FusedForm;
  if ((int)blockIdx.x >= nc) {
    // producer block b of spc: its slices of every chunk, chunk by chunk; one count per block and chunk
    const int b = (int)blockIdx.x - nc;
    if (fz.starve) return;                                                        // debug key "quad_starve": a producer that is never scheduled
    const int64_t per_chunk = (int64_t)fz.ch * a.C, total = (int64_t)a.n_traj * a.C;
    for (int chn = 0; chn < fz.nchunks; ++chn) {
      const int64_t base = (int64_t)chn * per_chunk, end = min(base + per_chunk, total);
      for (int sub = threadIdx.x; sub < QUAD_FUSED_NT; sub += NT)               // (NT = QUAD_FUSED_NT: once)
        for (int64_t idx = base + (int64_t)b * QUAD_FUSED_NT + sub; idx < end; idx += (int64_t)spc * QUAD_FUSED_NT)
          quad_fill_record<D>(a.ws_z, idx, a.C, a.traj_offset, a.seed, a.chain_offset, eig);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                          // this wave's records are acknowledged ...
      __syncthreads();                                                          // ... and so are the block's other waves' ...
      if (threadIdx.x == 0) __hip_atomic_fetch_add(fz.flags + chn, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ... before they are counted
    }
    return;
  }
  if constexpr (NI > 0) {
    constexpr int NS = quad_fused_ns(LB, true), NU = quad_nu(LB, NS, true);
    __shared__ float ring[NI * 2 * NU * 64];       // per integrating wave: two buffers of NU positions x 64 lanes
    const int wave = (int)(threadIdx.x >> 6), pair = wave < NI ? wave : wave - NI;
    const uint32_t lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)ring + (uint32_t)(pair * 2 * NU * 256) + (uint32_t)(threadIdx.x & 63) * 4u;
    const int64_t gt = ((int64_t)blockIdx.x * NI + pair) * 64 + (threadIdx.x & 63);
    if (wave >= NI) { quad_rows_body<D, LB, RowsForm>(a, eig, gt, lds); return; }
    __builtin_amdgcn_s_setprio(3);
    quad_body<D, LB, RowsForm>(a, eig, gt, fz, lds);
  } else {
    __builtin_amdgcn_s_setprio(3);                 // a consumer's time is its issue rate: it goes first where a producer shares its SIMD
    quad_body<D, LB, FusedForm>(a, eig, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, fz);
  }
  if (threadIdx.x == 0) {
    const uint32_t old = __hip_atomic_fetch_add(done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (old == (uint32_t)nc - 1u) {                                             // every consumer has read every chunk
      for (int i = 0; i < fz.nchunks; ++i) __hip_atomic_store(fz.flags + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(done, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
template <int D, int LB, int NI = 0>
__global__ __launch_bounds__(quad_fused_threads(NI)) void hmc_gauss_quad_fused_kernel(GaussArgs<float> a, const float* __restrict__ eig, QuadFused fz,
                                                                                      int nc, int spc, uint32_t* done) {
  quad_fused_block<D, LB, NI, false>(a, eig, fz, nc, spc, done);
}
// its propagator twin (quad_body: PROP): the same producers, counters and rings
template <int D, int NI = 0>
__global__ __launch_bounds__(quad_fused_threads(NI)) void hmc_gauss_quad_fused_prop_kernel(GaussArgs<float> a, const float* __restrict__ eig, QuadFused fz,
                                                                                           int nc, int spc, uint32_t* done) {
  quad_fused_block<D, QUAD_PROP_LB, NI, true>(a, eig, fz, nc, spc, done);
}


// LOCAL (tuning key "quad_local", default 1; D <= 3): the records of a block's chains are drawn by producer waves of THAT block and
// handed over through LDS - no record travels through memory, no chunk counter, no poll, no wait for chunk 0, and the launch does
// not depend on any other block being resident (the HAND-OVER FAILURE of QuadFused cannot happen: waves of one workgroup are
// co-resident by construction).  One block = 16 chains, four waves, one per SIMD:
//   wave 0     integrates (quad_body: ROWS, LOCAL): its record element is a ds_read_b32 at lane base + position x 256
//   wave 1     its row wave (quad_rows_body)
//   waves 2-3  produce: lane (position % 8, chain) computes quad_make_record's record - the cross-block producer's arithmetic - and
//              writes it with one 16-byte LDS write to [position][chain]
//   ring       next to the message ring, two record buffers of one pass (NU positions x 16 chains x 16 bytes)
//   hand-over  the barrier per group of the row-wave protocol, joined by the producers: while the integrator runs group g they fill
//              buffer (g + 1) % 2 with the records of group g + 1, and the barrier between the two groups publishes it; one more
//              barrier in front of the first group.  All roles walk quad_local_groups.
// Results are bit-identical to the cross-block launch (tests/test_gpu_quad_local.py).
// WIDE (quad_body: WIDE): element k of the record of position p goes to the integrating lane chain * 4 + k of block p >> 2, slot p & 3 -
// four dwords 16 bytes apart; a sweep of eight positions is two blocks.
// The sweep: lane `pl` of `nl` producer lanes draws positions pl / 16, + nl / 16, ... of a group for chain pl % 16 (128 lanes: eight
// positions of 16 chains per sweep); pl < 0: this wave draws nothing and only walks the groups.
// LEAD (hmc_gauss_quad_lead_kernel, tuning key "quad_lead"): the groups up to and including the launch's first full pass of NU are
// drawn with the sweep (pl_lead, nl_lead) - more lanes: the integrating wave waits for exactly these records with nothing to do -
// and the groups behind it with (pl, nl); both sweeps put a record where the integrating wave reads it.  pl_lead % 16 == pl % 16.
// INVARIANT: which lanes draw is the only thing a sweep decides.  Every wave that runs this function - drawing or not, chains past
// a.C or not, a launch shorter than one group or not - executes one "s_waitcnt lgkmcnt(0) ; s_barrier" per group of
// quad_local_groups, in that order, and the two closing barriers: the barrier sequence of every role is a function of the launch
// arguments alone, whatever the sweeps are.
// CPB (the propagator's 512-thread twin, quad_wide_block): the chains of a block, 16, 8 or 4.  A block's lanes of chain slots >= CPB
// are switched off like lanes past a.C, nobody draws for them, and a producer lane's share becomes (position l / CPB, chain l % CPB):
// with four chains 128 lanes cover the 32 positions of a pass in ONE sweep.
template <int D, int LB, typename Form, int CPB = 16>
__device__ __forceinline__ void quad_local_produce(const GaussArgs<float>& a, const float* __restrict__ eig, const int64_t c0, const uint32_t recl,
                                                   const int pl, const int nl, const int pl_lead, const int nl_lead) {
  constexpr int NS = quad_fused_ns(LB, true), NU = quad_nu(LB, NS, true);
  static_assert(Form::LOCAL && rec_elems<float, D>() == 4, "the local launch's producers: one 16-byte record");
  constexpr bool WIDE = Form::WIDE;
  typedef float V4f __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) V4f* lvec_t;
  typedef __attribute__((address_space(3))) float* lflt_t;
  (void)(lvec_t)nullptr;
  static_assert(CPB == 16 || CPB == 8 || CPB == 4, "a power of two of chain slots; sweeps of 64 k lanes stay whole blocks of four positions");
  constexpr int CS = CPB == 16 ? 4 : (CPB == 8 ? 3 : 2);                       // log2 CPB
  const int chain = pl_lead & (CPB - 1);
  const int64_t c = min(c0 + chain, a.C - 1);                                   // (past a.C: the last chain again, as the integrator does)
  const uint64_t gchain = a.chain_offset + (uint64_t)c;
  uint32_t buf = recl;                                                          // the record buffer being filled
  const uint32_t buf_both = 2u * recl + (uint32_t)(NU * 256);
  bool lead = true;
  quad_local_groups<NS, NU>(a, [&](int t0, int, auto G, auto) {
    const int l = lead ? pl_lead : pl, step = (lead ? nl_lead : nl) >> CS;      // (step: a multiple of four positions - whole blocks of WIDE)
    const int p0 = l >= 0 ? l >> CS : NU;                                       // (NU: past every group)
    const uint32_t dst = buf + (WIDE ? (uint32_t)((p0 >> 2) * 1024 + chain * 64 + (p0 & 3) * 4) : (uint32_t)(p0 * 256 + chain * 16));
    for (int p = p0; p < decltype(G)::value; p += step) {                       // (p < NU: inside the buffer)
      float rec[4];
      quad_make_record<D>(a.seed, gchain, (uint32_t)(a.traj_offset + t0 + p), eig, rec);
      if constexpr (WIDE) {
        const lflt_t w = (lflt_t)(uintptr_t)(dst + (uint32_t)((p - p0) * 256));      // (four positions on: one block of 1024 bytes)
        w[0] = rec[0]; w[4] = rec[1]; w[8] = rec[2]; w[12] = rec[3];
      } else {
        *(lvec_t)(uintptr_t)(dst + (uint32_t)((p - p0) * 256)) = V4f{rec[0], rec[1], rec[2], rec[3]};
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");          // publishes this group's records
    buf = buf_both - buf;
    if (decltype(G)::value == NU) lead = false;
  });
  asm volatile("s_barrier\n\ts_barrier" ::: "memory");                          // the last group's hand-over and the status message: the other roles'
}
template <int D, int LB, bool PROP>
__device__ __forceinline__ void quad_local_block(const GaussArgs<float>& a, const float* __restrict__ eig, int wt) {
  typedef std::conditional_t<PROP, QuadPropOf<QuadLocalForm>, QuadLocalForm> Form;
  constexpr int NS = quad_fused_ns(LB, true), NU = quad_nu(LB, NS, true);
  __shared__ __attribute__((aligned(16))) float ring[2 * NU * 64 + 2 * NU * 64];      // messages (64 lanes x 4 bytes) | records (16 chains x 16 bytes), two passes each
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const uint32_t msgs = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)ring, recs = msgs + (uint32_t)(2 * NU * 256);
  const int64_t gt = (int64_t)blockIdx.x * 64 + lane;
  if (wave == 0) {
    __builtin_amdgcn_s_setprio(3);
    quad_body<D, LB, Form>(a, eig, gt, QuadFused{nullptr, 1, 0u, 0, nullptr, 0}, msgs + (uint32_t)lane * 4u, recs + (uint32_t)lane * 4u);
  }
  else if (wave == 1) quad_rows_body<D, LB, Form>(a, eig, gt, msgs + (uint32_t)lane * 4u, wt != 0);
  else quad_local_produce<D, LB, Form>(a, eig, (int64_t)blockIdx.x * 16, recs, (int)threadIdx.x - 128, 128, (int)threadIdx.x - 128, 128);
}
template <int D, int LB>
__global__ __launch_bounds__(256) void hmc_gauss_quad_local_kernel(GaussArgs<float> a, const float* __restrict__ eig, int wt) {
  quad_local_block<D, LB, false>(a, eig, wt);
}
template <int D>
__global__ __launch_bounds__(256) void hmc_gauss_quad_local_prop_kernel(GaussArgs<float> a, const float* __restrict__ eig, int wt) {
  quad_local_block<D, QUAD_PROP_LB, true>(a, eig, wt);
}
// WIDE (tuning key "quad_wide"): the local launch - the same roles, rings of the same sizes, the same groups and barriers - with
// 16-byte hand-overs per block of four positions (quad_body: WIDE); a lane's base in a block of either ring is lane x 16 bytes.
// Results are bit-identical to the local launch (tests/test_gpu_quad_wide.py).
// LEAD (tuning key "quad_lead", hmc_gauss_quad_lead_kernel): the wide launch with 512 threads.  The launch's lead-in is the time the
// producers need for the first full pass - 32 positions x 16 chains, four sweeps of waves 2-3 - while the integrating wave, done
// with the lead group after one eighth of that, and the row wave stand at a barrier.  Waves 4-7 draw their share of the groups
// up to and including that pass (quad_local_produce: LEAD): 384 lanes, 24 positions per sweep, waves 4-5 (the SIMDs of the two
// idle roles) first in the sweep, so the pass is two wave-sweeps on each SIMD instead of four on two.  Behind it they draw
// nothing and walk the groups to the end with everybody's barriers; they never leave early.  Same records in the same places:
// results are bit-identical to the 256-thread launch (tests/test_gpu_quad_lead.py).
// PROP twins (hmc_gauss_quad_wide_prop_kernel, hmc_gauss_quad_lead_prop_kernel).  A propagated trajectory is ~20 instructions on
// the integrating wave, a record ~290 on a producer lane: the two producer waves of the step-by-step launch (eight positions of
// 16 chains per sweep) no longer keep up, and 64 blocks leave three quarters of the chip without a record to draw.  The 512-thread
// twin therefore runs with CPB = 4 chains per block up to 1024 chains (tuning key "quad_prop_chains"; quad_local_produce: CPB):
// waves 2-3 cover a pass of 32 positions in one sweep, on SIMDs that hold neither the integrating wave nor the row wave.  Measured
// (profiles/r16a_quad_prop.txt): producers that draw nothing are not faster - the integrating wave's issue binds.
// SWEEP (tuning key "quad_prop_sweep", default 0, the 512-thread twin only) names the waves that draw
// BEHIND the first full pass: 0 = waves 2-3 as before, 1 = waves 2, 3, 6, 7 (256 lanes, 16 positions per sweep: two drawing waves
// on each of the two SIMDs that hold neither the integrating wave nor the row wave), 2 = waves 2-7 (384 lanes, the lead-in's
// sweep).  Which lanes draw is all a sweep decides (quad_local_produce: INVARIANT): every wave walks every group and barrier.
template <int D, int LB, bool LEAD, bool PROP = false, int CPB = 16>
__device__ __forceinline__ void quad_wide_block(const GaussArgs<float>& a, const float* __restrict__ eig, const bool wt, const int sweep = 0) {
  typedef std::conditional_t<PROP, QuadPropOf<QuadWideForm>, QuadWideForm> Form;
  constexpr int NS = quad_fused_ns(LB, true), NU = quad_nu(LB, NS, true);
  static_assert(NS == 4 && NU % 4 == 0, "groups are whole blocks of four positions, or single ones");
  __shared__ __attribute__((aligned(16))) float ring[2 * NU * 64 + 2 * NU * 64];      // as the local launch's: messages | records, two passes each
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const uint32_t msgs = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)ring, recs = msgs + (uint32_t)(2 * NU * 256);
  const int64_t gt = CPB == 16 || lane < 4 * CPB ? (int64_t)blockIdx.x * (4 * CPB) + lane : a.C * 4;      // (a chain slot >= CPB: off, like a chain past a.C)
  if (wave == 0) {
    __builtin_amdgcn_s_setprio(3);
    quad_body<D, LB, Form>(a, eig, gt, QuadFused{nullptr, 1, 0u, 0, nullptr, 0}, msgs + (uint32_t)lane * 16u, recs + (uint32_t)lane * 16u);
  }
  else if (wave == 1) quad_rows_body<D, LB, Form>(a, eig, gt, msgs + (uint32_t)lane * 16u, wt);
  else if constexpr (LEAD) {
    const int lw = wave < 4 ? wave : (wave < 6 ? wave - 4 : wave - 2);               // place in the lead sweep: waves 4 5 2 3 6 7
    int pl = wave < 4 ? (int)threadIdx.x - 128 : -1, nl = 128;                         // the sweep behind the first full pass
    if (PROP && sweep == 1) { pl = wave < 4 ? (int)threadIdx.x - 128 : (wave >= 6 ? (int)threadIdx.x - 256 : -1); nl = 256; }
    if (PROP && sweep == 2) { pl = lw * 64 + lane; nl = 384; }
    quad_local_produce<D, LB, Form, CPB>(a, eig, (int64_t)blockIdx.x * CPB, recs, pl, nl, lw * 64 + lane, 384);
  }
  else quad_local_produce<D, LB, Form, CPB>(a, eig, (int64_t)blockIdx.x * CPB, recs, (int)threadIdx.x - 128, 128, (int)threadIdx.x - 128, 128);
}
template <int D>
__global__ __launch_bounds__(256) void hmc_gauss_quad_wide_prop_kernel(GaussArgs<float> a, const float* __restrict__ eig, int wt) {
  quad_wide_block<D, QUAD_PROP_LB, false, true>(a, eig, wt != 0);
}
template <int D, int CPB>
__global__ __launch_bounds__(512) void hmc_gauss_quad_lead_prop_kernel(GaussArgs<float> a, const float* __restrict__ eig, int wt, int sweep) {
  quad_wide_block<D, QUAD_PROP_LB, true, true, CPB>(a, eig, wt != 0, sweep);
}
template <int D, int LB>
__global__ __launch_bounds__(256) void hmc_gauss_quad_wide_kernel(GaussArgs<float> a, const float* __restrict__ eig, int wt) {
  quad_wide_block<D, LB, false>(a, eig, wt != 0);
}
template <int D, int LB>
__global__ __launch_bounds__(512) void hmc_gauss_quad_lead_kernel(GaussArgs<float> a, const float* __restrict__ eig, int wt) {
  quad_wide_block<D, LB, true>(a, eig, wt != 0);
}

}  // namespace hta
