// Matrix-core metric kernel: the general sequence of one evaluation (metric_warm_system) and the out-of-line evaluations the two kernels
// call - warm_general_eval, traj_general_eval - which read their arguments again from the kernel-argument segment; traj_select.
#pragma once
#include "rmhmc.hpp"
#include "rmhmc_metric_mfma_fast_dev.hpp"

namespace hta {

// The bits of `second`, the kernels' last argument: what the tuning keys select (metric_second_bits() on the host), and two that the device
// code sets on the way down.
constexpr int kSecClosed = 1;          // "metric_second": the refinement's second pass in closed form - and with it the fast solve
constexpr int kSecBf16 = 2;            // "metric_bx3" >= 1: the fast solve's second product F E1 as three bfloat16 products
constexpr int kSecResident = 4;        // "metric_resident": the trajectory kernel keeps the state in LDS in eigen-coordinates
constexpr int kSecCallerRotates = 8;   // set by the resident trajectory loop: the caller does the copies / the binding rotation itself
constexpr int kSecSqrtDraw = 16;       // "metric_sqrtdraw": the momentum draw as p = G^(1/2) z
constexpr int kSecFastDeclined = 32;   // set by metric_warm_mfma_kernel: it has tried the fast solve itself and it declined
constexpr int kSecBf16Form = 64;       // "metric_bx3" >= 2: the fast solve's formation on bfloat16 as well

// One evaluation of system b (everything of the file's header); the workgroup's 1024 threads, state in the dynamic LDS block.
// `vres`: the matrix buffer (offset) that holds the staged shared basis V0 on entry, or -1; on return, the buffer that holds it
// now (a solve ends with V0 staged for x = V0 x': the next evaluation of a trajectory kernel starts from that copy), or -1.
__device__ __forceinline__ void metric_warm_system(const MetricArgsT<float>& a, int DP, int LD, int64_t b, int& vres, int second, int tiles) {      // second: the kSec* bits
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int D = a.D, tid = threadIdx.x;
  const int nt = DP / 16, k4 = (D + 3) / 4;
  const int ne = D + (D & 1);
  float* const lds0 = reinterpret_cast<float*>(smem_raw);
  const MetricLds lay(DP, LD);
  const int oB0 = 0, oB1 = lay.oB1, oB2 = lay.oB2;
  const int oJit = lay.oJit, oLam = lay.oLam, oLt = lay.oLt, oM = lay.oM, oY = lay.oY, oX = lay.oX, oD = lay.oD, oRed = lay.oRed, oW = lay.oW;
  float* vjit = lds0 + oJit; float* vlam = lds0 + oLam; float* vlt = lds0 + oLt; float* vm = lds0 + oM; float* vy = lds0 + oY;
  float* vx = lds0 + oX; float* vd = lds0 + oD; float* red = lds0 + oRed;
  const bool softabs = a.metric == 1;
  // GENERAL mode (round 3): every system has its own curvature Hs_b AND its own approximate eigenbasis V0_b (the caller's
  // previous evaluation at that chain): A = V0_b^T (Hs_b + diag(e)) V0_b by two products, the refinement where its coupling
  // test passes, the in-launch Jacobi (on the nearly diagonal A: few sweeps) where it does not; V_out = V0_b X is the
  // basis for the caller's next call.  lam0 is not used.
  const bool general = softabs && a.hs_stride != 0;
  // the momentum draw as a solve-shaped evaluation (tuning key "metric_sqrtdraw"): p = G^(1/2) z = Q diag(sqrt lam~) Q^T z - same law as chol(G) z
  const bool sdraw = (second & kSecSqrtDraw) && a.p_out && softabs && !general && !a.m && !a.G_out && !a.V_out && !a.dmetric_out;
  const bool has_m = a.m || sdraw;
  if (!(second & kSecFastDeclined) && (second & kSecClosed) && softabs && !general && has_m && !(a.G_out || (a.p_out && !sdraw) || a.V_out || a.dmetric_out) && (!a.X || a.Pm == a.Hs)) {
    if (metric_fast_solve(a, DP, LD, b, vres, (second & kSecBf16) != 0, tiles, -1, 0, sdraw, (second & kSecBf16Form) != 0)) return;
  }

  {
    const uint64_t chain = a.chain_offset + (uint64_t)b;
    const float* V0b = a.V0 + (general ? b * a.v0_stride : 0);
    __syncthreads();
    // ---- 0. operands: jitter, the solve vector, d = X - mu; V0 into LDS
    if (tid < DP) {
      const int i = opaque_tid();
      vjit[i] = (i < D && a.has_jitter) ? (float)a.jitter * uniform_elem<float>(a.seed, chain, a.draw, PURPOSE_JITTER, a.sub, i) : 0.f;
      vm[i] = (i < D && has_m) ? (sdraw ? normal_elem<float>(a.seed, a.chain_offset + (uint64_t)b, a.draw, 0, i) : a.m[b * D + i]) : 0.f;
      vd[i] = (i < D && a.X) ? a.X[b * D + i] - a.mu[i] : 0.f;
    }
    // buffer roles: bx = V0 (then X), by = A / S / E, bz = scratch
    int bx = oB1, by = oB0, bz = oB2;
    const bool resident = softabs && !general && vres >= 0;
    if (resident) { bx = vres; by = vres == oB0 ? oB1 : oB0; bz = vres == oB2 ? oB1 : oB2; }
    vres = -1;
    if (softabs && !resident) ph_stage(V0b, bx, D, DP, LD);
    __syncthreads();
    // ---- Gaussian log-prob and P (X - mu)
    float logp = 0.f;
    if (a.X) logp = (float)a.log_norm - 0.5f * ph_logp(a.Pm, oD, D, bz, oRed, a.upd_g ? a.upd_g + b * D : nullptr, (float)a.cg);
    // ---- m' = V0^T m
    if (has_m && softabs) {
      const float v = ph_mv8(1, bx, LD, oM, D);
      __syncthreads();
      if ((tid & 7) == 0 && (tid >> 3) < DP) vm[tid >> 3] = ((tid >> 3) < D) ? v : 0.f;
    }
    // ---- 1. A = diag(lam0) + V0^T diag(e) V0 into buffer 0 (symmetric, zero padded); general: A = V0^T (Hs + diag(e)) V0 into buffer 2
    if (softabs && !general) {
      lds_gemm<true, false, true, true>(bx, bx, by, -1, oJit, nt, k4, LD);
      __syncthreads();
      { const int i = opaque_tid(); if (i < D) lds0[by + i * LD + i] += a.lam0[i]; }
    } else if (general) {
      ph_stage_sym(a.Hs + b * a.hs_stride, oB2, oJit, D, DP, LD);
      __syncthreads();
      lds_gemm<false, false, false, false>(oB2, oB1, oB0, -1, -1, nt, k4, LD);          // T = (Hs + diag e) V0
      __syncthreads();
      lds_gemm<true, false, true, false>(oB1, oB0, oB2, -1, -1, nt, k4, LD);            // A = V0^T T
      by = oB2; bz = oB0;
    }
    __syncthreads();
    // ---- 2. eigenvectors X of A by iterative refinement from X = I; bx: X, by: A / S / E, bz: scratch
    bool have_x = false, converged = false, fallback = !softabs;     // Metric.HESSIAN: G = A, no decomposition needed
    float emax_prev = 1.f;
    bool implicit_e = false;          // the last update X (I + E) is applied to the vectors of the solve instead of being formed
    bool x_antisym = false;           // X = I + E1 straight from the first pass: X + X^T = 2 I exactly (the pairs), so X^T v = 2 v - X v
    bool et_in_bz = false;            // the closed-form second pass left E2^T in bz (next to E2 in by)
    const bool want_matrix = a.G_out || (a.p_out && !sdraw) || a.V_out || a.dmetric_out;
    if (softabs) {
      for (int it = 0; it < 4 && !converged && !fallback; ++it) {
        if (it >= 2 && general) { fallback = true; break; }          // (forming A again needs all three buffers: the Jacobi path does it)
        if (it >= 2) {                                               // rare: A was consumed by the previous pass, form it again
          ph_stage(a.V0, bz, D, DP, LD);
          __syncthreads();
          lds_gemm<true, false, true, true>(bz, bz, by, -1, oJit, nt, k4, LD);
          __syncthreads();
          if (tid < D) lds0[by + tid * LD + tid] += a.lam0[tid];
          __syncthreads();
        }
        float emax;
        if (it == 1 && have_x && (second & kSecClosed) && emax_prev <= kSecondE) {
          // second pass in closed form: M = F E1 (F = A, E1 = X without their diagonals), then ph_refine_E2
          { const int i = opaque_tid(); if (i < D) { lds0[by + i * LD + i] = 0.f; lds0[bx + i * LD + i] = 0.f; } }
          __syncthreads();
          lds_gemm<false, false, false, false>(by, bx, bz, -1, -1, nt, k4, LD);       // M = F E1
          __syncthreads();
          emax = ph_refine_E2(bz, bx, by, oLam, oRed, D, LD);
          et_in_bz = true;
        } else {
          if (have_x) {
            lds_gemm<false, false, false, false>(by, bx, bz, -1, -1, nt, k4, LD);     // T = A X
            __syncthreads();
            lds_gemm<true, false, true, false>(bx, bz, by, -1, -1, nt, k4, LD);       // S = X^T T
            __syncthreads();
            lds_gemm<true, false, true, false>(bx, bx, bz, -1, -1, nt, k4, LD);       // Gm = X^T X
            __syncthreads();
          }
          // first pass: X = I + E goes next to A (still needed for A X); later passes: E in place of S
          emax = ph_refine_E(by, bz, have_x ? by : bx, oLam, oRed, have_x ? 1 : 0, D, LD);
        }
        emax_prev = emax;
        if (emax > kFallbackE) { fallback = true; break; }
        __syncthreads();
        if (have_x && !want_matrix && emax <= kConvE) {
          // the converging pass of an evaluation that only solves: X2 = X (I + E) enters through X2^T m' = (I + E^T) X^T m'
          // and X2 w = X (w + E w) - four matrix-vector products instead of one D^3 product (14.8 k of 116 k cycles at cfg3)
          implicit_e = true; converged = true;
          break;
        }
        if (have_x) {
          lds_gemm<false, false, false, false>(bx, by, bz, bx, -1, nt, k4, LD);       // X <- X + X E
          __syncthreads();
          const int t = bx; bx = bz; bz = t;
          x_antisym = false; et_in_bz = false;
        } else {
          have_x = true;                                                              // bx = I + E, by = A still
          x_antisym = true;
        }
        converged = emax <= kConvE;
      }
      if (!converged) fallback = true;
      if (fallback) {
        // cyclic Jacobi on A (rmhmc_metric_dev.hpp): no assumption on gaps or perturbation size
        __syncthreads();
        if (general) {                                               // A again: V0 -> bx, Hs -> bz, T -> by, A -> bz; then A lives in `by`
          ph_stage(V0b, bx, D, DP, LD);
          ph_stage_sym(a.Hs + b * a.hs_stride, bz, oJit, D, DP, LD);
          __syncthreads();
          lds_gemm<false, false, false, false>(bz, bx, by, -1, -1, nt, k4, LD);
          __syncthreads();
          lds_gemm<true, false, true, false>(bx, by, bz, -1, -1, nt, k4, LD);
          const int t = by; by = bz; bz = t;
        } else {
          ph_stage(a.V0, bz, D, DP, LD);
          __syncthreads();
          lds_gemm<true, false, true, true>(bz, bz, by, -1, oJit, nt, k4, LD);
          __syncthreads();
          if (tid < D) lds0[by + tid * LD + tid] += a.lam0[tid];
        }
        __syncthreads();
        for (int e = tid; e < DP * LD; e += MT) { const int i = e / LD, j = e - i * LD; lds0[bz + e] = (i == j && i < D) ? 1.f : 0.f; }
        __syncthreads();
        jacobi_fallback(by, bz, D, ne, LD, oJit, oRed, a.max_sweeps);
        if (tid < D) vlam[tid] = lds0[by + tid * LD + tid];
        for (int e = tid; e < DP * LD; e += MT) { const int i = e / LD, j = e - i * LD; lds0[bx + e] = (i < D && j < D) ? lds0[bz + j * LD + i] : 0.f; }   // X[i][k] = VT[k][i]
        __syncthreads();
      }
    }
    // ---- 3. soft-abs map, log-determinant  (S:120, S:726)
    float logdet = 0.f, quad = 0.f;
    if (softabs) {
      float ld = 0.f;
      if (tid < DP) {
        const int i = opaque_tid();
        float lt = 1.f;
        if (i < D) {
          const float lam = vlam[i];
          lt = (1.f / tanhf((float)a.alpha * lam)) * lam;
          ld = logf(lt);
          if (a.lam_out) a.lam_out[b * D + i] = lt;
          if (a.lamraw_out) a.lamraw_out[b * D + i] = lam;
        }
        vlt[i] = lt;
      }
      logdet = block_sum_dpp(ld, red);
      // ---- 4. x = V0 X (X^T m' / lam~)
      if (has_m) {
        // y = X^T m': row-wise products only where the structure allows it (mv8: a third of the column-wise product's time)
        float y;
        const int row = opaque_tid() >> 3;
        if (x_antisym && !fallback) { const float xm = ph_mv8(0, bx, LD, oM, D); y = 2.f * vm[row < DP ? row : 0] - xm; }
        else y = ph_mv8(1, bx, LD, oM, D);
        if (implicit_e) {                                       // y <- (I + E^T) y
          __syncthreads();
          if ((tid & 7) == 0 && row < DP) vy[row] = (row < D) ? y : 0.f;
          __syncthreads();
          y += et_in_bz ? ph_mv8(0, bz, LD, oY, D) : ph_mv8(1, by, LD, oY, D);
          __syncthreads();
        }
        float qd = 0.f;
        float wreg = 0.f;
        if ((tid & 7) == 0 && row < DP) {
          const float w = (row < D) ? (sdraw ? y * sqrtf(vlt[row]) : y / vlt[row]) : 0.f;
          wreg = w;
          (implicit_e ? vx : vy)[row] = w;
          qd = (row < D) ? y * w : 0.f;
        }
        quad = block_sum_dpp(qd, red);
        if (implicit_e) {                                       // w <- w + E w
          const float ew = ph_mv8(0, by, LD, oX, D);
          __syncthreads();
          if ((tid & 7) == 0 && row < DP) vy[row] = (row < D) ? wreg + ew : 0.f;
          __syncthreads();
        }
        const float xp = ph_mv8(0, bx, LD, oY, D);
        __syncthreads();
        if ((tid & 7) == 0 && row < DP) vx[row] = (row < D) ? xp : 0.f;
        __syncthreads();
        ph_stage(V0b, by, D, DP, LD);                           // (the E buffer is dead)
        __syncthreads();
        if (!general) vres = by;
        const float x = ph_mv8(0, by, LD, oX, D);
        const int orow = opaque_tid() >> 3;
        if ((tid & 7) == 0 && orow < D) {
          if (sdraw) a.p_out[b * D + orow] = x;
          if (a.x_out) a.x_out[b * D + orow] = x;
          if (a.upd_x) a.upd_x[b * D + orow] += (float)a.cx * x;
        }
      }
    }
    // ---- 4b. the eigenbasis itself (V_out: the next call's warm start) and the derivative matrix M = Q W Q^T (dmetric_out)
    bool q_ready = false;
    if (softabs && (a.V_out || a.dmetric_out)) {
      vres = -1;
      __syncthreads();
      if (!has_m && tid < DP) vy[tid] = 0.f;                            // u = Q^T m / lam~ (vy holds it after the solve)
      ph_stage(V0b, by, D, DP, LD);
      __syncthreads();
      lds_gemm<false, false, false, false>(by, bx, bz, -1, -1, nt, k4, LD);             // Q = V0 X
      __syncthreads();
      if (a.V_out) {
        // a system that went non-finite (a diverged chain: NaN curvature, or a NaN basis handed in) must not poison its NEXT
        // evaluation: its basis restarts from the identity
        if (!(fabsf(logdet) <= 3.0e38f)) {
          __attribute__((address_space(1))) float* vg = (__attribute__((address_space(1))) float*)(a.V_out + b * D * D);
          for (int e = tid; e < D * D; e += MT) vg[e] = (e / D == e % D) ? 1.f : 0.f;
        } else {
          ph_store_dense(a.V_out + b * D * D, bz, D, LD);
        }
      }
      if (a.dmetric_out) {
        ph_dmetric_w(by, oLam, oLt, oY, (float)a.alpha, D, DP, LD);
        __syncthreads();
        lds_gemm<false, true, false, false>(by, bz, bx, -1, -1, nt, k4, LD);            // T = W Q^T
        __syncthreads();
        lds_gemm<false, false, true, false>(bz, bx, by, -1, -1, nt, k4, LD);            // M = Q T (symmetric)
        __syncthreads();
        ph_store_dense(a.dmetric_out + b * D * D, by, D, LD);
        __syncthreads();
      } else {
        q_ready = true;                                               // bz = Q, bx = X still: step 5 must not stage V0 again (V_out may alias it)
      }
    }
    // ---- 5. G = Q diag(lam~) Q^T, Q = V0 X  (S:121) for fisher() / the momentum draw; Metric.HESSIAN: G = Hs itself
    if (a.G_out || (a.p_out && !sdraw) || !softabs) {
      vres = -1;
      __syncthreads();
      int g = bz;
      if (softabs) {
        if (!q_ready) {
          ph_stage(V0b, by, D, DP, LD);
          __syncthreads();
          lds_gemm<false, false, false, false>(by, bx, bz, -1, -1, nt, k4, LD);       // Q = V0 X
        }
        __syncthreads();
        lds_gemm<false, true, true, true>(bz, bz, by, -1, oLt, nt, k4, LD);           // G = Q (diag(lam~) Q^T)
        g = by;
      } else {
        const float* Hs = a.Hs + b * a.hs_stride;
        for (int e = tid; e < DP * LD; e += MT) {
          const int i = e / LD, j = e - i * LD;
          float v = 0.f;
          if (i < D && j < D) { v = (i >= j) ? Hs[i * D + j] : Hs[j * D + i]; if (i == j) v += vjit[i]; }
          lds0[g + e] = v;
        }
      }
      __syncthreads();
      if (a.G_out) for (int e = tid; e < D * D; e += MT) { const int i = e / D, j = e - i * D; a.G_out[b * D * D + e] = lds0[g + i * LD + j]; }
      if (a.p_out || !softabs) {
        mfma_cholesky(g, D, DP, LD, oW);
        if (!softabs) {
          float ld = 0.f;
          if (tid < D) ld = 2.f * logf(lds0[g + tid * LD + tid]);                     // slogdet (S:728) for a PD metric
          logdet = block_sum_dpp(ld, red);
          if (a.m) {
            if (tid < D) { vy[tid] = a.m[b * D + tid]; vx[tid] = vy[tid]; }
            ph_chol_solve(g, D, LD, oY);
            float qd = 0.f;
            if (tid < D) {
              qd = vx[tid] * vy[tid];
              if (a.x_out) a.x_out[b * D + tid] = vy[tid];
              if (a.upd_x) a.upd_x[b * D + tid] += (float)a.cx * vy[tid];
            }
            quad = block_sum_dpp(qd, red);
          }
        }
        if (a.p_out) {                   // p = L z  (S:184 via MultivariateNormal.rsample)
          __syncthreads();
          if (tid < DP) vd[tid] = (tid < D) ? normal_elem<float>(a.seed, chain, a.draw, 0, tid) : 0.f;
          __syncthreads();
          const float p = ph_mv8_lower(g, LD, oD, D);
          const int prow = opaque_tid() >> 3;
          if ((tid & 7) == 0 && prow < D) a.p_out[b * D + prow] = p;
        }
      }
    }
    if (tid == 0) {
      if (a.logdet_out) a.logdet_out[b] = logdet;
      if (a.quad_out) a.quad_out[b] = quad;
      if (a.logp_out) a.logp_out[b] = logp;
      if (a.H_out) {
        const float pi_term = (float)D * 1.8378770351409912f;                            // S:712 in float32
        a.H_out[b] = -logp + 0.5f * pi_term + 0.5f * logdet + 0.5f * quad;               // S:731
      }
    }
  }
}

// The evaluations of a trajectory that are NOT the fast solve - the momentum draw, every evaluation of the form that keeps the state in the
// caller's coordinates, the resident form's rare way out - run out of line and read the kernel's arguments again from the kernel-argument
// segment: inlined into the kernel they kept all ~90 argument dwords live across the resident loop (404 scalar registers parked in vector
// lanes, a v_readlane per use - and with 16 waves on the CU every instruction a wave executes costs the workgroup 16 cycles).
// op: the evaluation's index in the trajectory (0 draw, 1 H_old, 2 .. 4 L + 1 half steps, 4 L + 2 H_new); mode 0: the state in global memory
// (t.th / t.pm / t.thc / t.pmc), the copies / the binding rotation after the evaluation included; mode 1: the state is resident in LDS in
// eigen-coordinates - state out, evaluation, state in.  Returns the buffer that holds V0 afterwards (-1: none).
constexpr int kTrajArgOff = (int)((sizeof(MetricArgsT<float>) + 7) / 8 * 8);
typedef const __attribute__((address_space(4))) char* kernarg_ptr;
// (the segment pointer is read in the KERNEL and handed down: __builtin_amdgcn_kernarg_segment_ptr() in a called function returned null here)
template <typename S> __device__ __forceinline__ S load_kernarg(kernarg_ptr ka, int off) {      // dword by dword from the constant address space: scalar loads
  S v;
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const __attribute__((address_space(4))) uint32_t* kp;
  kp src = (kp)(ka + off);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(S) / 4); ++i) dst[i] = src[i];
#else
  memset(&v, 0, sizeof(v));
#endif
  return v;
}
// the pointer as a callee sees it - an argument arrives in vector registers - made uniform again: the loads above stay scalar
__device__ __forceinline__ kernarg_ptr uniform_kernarg(kernarg_ptr ka) {
  const uint64_t u = (uint64_t)ka;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return (kernarg_ptr)(((uint64_t)hi << 32) | lo);
}
static_assert(alignof(MetricTrajArgs) == 8 && alignof(MetricArgsT<float>) == 8, "kernel-argument layout of metric_traj_mfma_kernel");
// one evaluation on the general sequence for metric_warm_mfma_kernel, out of line, its arguments read again from the kernel-argument segment (see
// traj_general_eval): the kernel's own body keeps only what the fast solve reads
__device__ __attribute__((noinline)) void warm_general_eval(kernarg_ptr ka, int DP, int LD, int64_t b, int vres, int second, int tiles) {
  ka = uniform_kernarg(ka);
  const MetricArgsT<float> a = load_kernarg<MetricArgsT<float>>(ka, 0);
  DP = HTA_U(DP); LD = HTA_U(LD); vres = HTA_U(vres); second = HTA_U(second);
  metric_warm_system(a, DP, LD, b, vres, second, tiles);
}

__device__ __attribute__((noinline)) int traj_general_eval(kernarg_ptr ka, int DP, int LD, int64_t b, int vres, int op, int second, int tiles, int mode) {
  ka = uniform_kernarg(ka);
  const MetricArgsT<float> a = load_kernarg<MetricArgsT<float>>(ka, 0);
  const MetricTrajArgs t = load_kernarg<MetricTrajArgs>(ka, kTrajArgOff);
  DP = HTA_U(DP); LD = HTA_U(LD); vres = HTA_U(vres); op = HTA_U(op); second = HTA_U(second); mode = HTA_U(mode);
  const int D = a.D, nops = 4 * t.L + 3;
  const TrajLds lay(DP, LD);
  const int BS = lay.BS, oY = lay.oY, sTh = lay.sTh, sP = lay.sP, sThc = lay.sThc, sPc = lay.sPc;
  MetricArgsT<float> o = a;
  // (the decode of `op` is written out here and in the resident loop of metric_traj_mfma_kernel, which sets sub / H_out / logp_out / cx / cg the same
  // way and leaves the operands to the resident vectors: the two must agree)
  int j = -1;
  if (op == 0) { o.sub = 0; o.p_out = t.pm; }                                                  // gibbs: p ~ N(0, G(theta))  S:183-184
  else if (op == 1) { o.sub = 1; o.X = mode ? t.th : t.cur; o.m = t.pm; o.H_out = t.H0; }      // H_old  S:971
  else if (op == nops - 1) { o.sub = 2u + 8u * (uint32_t)t.L; o.X = t.th; o.m = t.pm; o.H_out = t.H1; o.logp_out = t.lp1; }   // H_new  S:989
  else {
    const int q = op - 2, l = q >> 2;
    j = q & 3;
    const bool fa = j == 0 || j == 3;                                                          // phi_A/2 (S:429-430, S:457-458) : phi_B/2
    o.sub = 2u + 8u * (uint32_t)l + (j == 0 ? 1u : j == 1 ? 2u : j == 2 ? 4u : 7u);
    o.X = fa ? t.th : t.thc; o.m = fa ? t.pmc : t.pm; o.upd_x = fa ? t.thc : t.th; o.upd_g = fa ? t.pm : t.pmc;
    o.cx = t.eh; o.cg = -t.eh;
  }
  const int64_t e0 = b * D;
  if (mode == 1) {
    __syncthreads();
    if (vres < 0) { ph_stage(a.V0, BS, D, DP, LD); vres = BS; __syncthreads(); }
    ph_res_out(vres, sTh, sP, t.th + e0, t.pm + e0, a.mu, D, DP, LD);
    ph_res_out(vres, sThc, sPc, t.thc + e0, t.pmc + e0, a.mu, D, DP, LD);
    __syncthreads();
    metric_warm_system(o, DP, LD, b, vres, second & kSecBf16, tiles);                          // (kSecClosed off: not the fast solve again)
    __syncthreads();
    if (vres < 0) { ph_stage(a.V0, BS, D, DP, LD); vres = BS; }
    res_in(vres, oY, sTh, sP, t.th + e0, t.pm + e0, a.mu, D, DP, LD);
    res_in(vres, oY, sThc, sPc, t.thc + e0, t.pmc + e0, a.mu, D, DP, LD);
    return vres;
  }
  metric_warm_system(o, DP, LD, b, vres, second, tiles);
  if ((op == 1 || j == 1) && !(second & kSecCallerRotates)) {
    __syncthreads();
    const int i = opaque_tid();
    if (i < D) {
      const int64_t e = e0 + i;
      if (op == 1) {                                                                           // S:425-426
        const float x = t.cur[e];
        t.th[e] = x; t.thc[e] = x; t.pmc[e] = t.pm[e];
      } else {
        phi_c_elem<float>(t.th[e], t.pm[e], t.thc[e], t.pmc[e], t.c, t.s);                     // phi_C  S:447-450
      }
    }
  }
  return vres;
}

// The chain's Metropolis selection at the end of its trajectory (mh_select_kernel's rule, uniform and writes - hmc_pieces.hip - by the chain's own
// workgroup: the proposal t.th and the three scalars were written by this workgroup, visible after the barrier)
__device__ __forceinline__ void traj_select(const MetricArgsT<float>& a, const MetricTrajArgs& t, int64_t b) {
  __syncthreads();
  const int D = a.D, j = opaque_tid();
  const uint64_t chain = a.chain_offset + (uint64_t)b;
  const float u = u23<float>(philox_block(a.seed, chain, (uint32_t)t.n, PURPOSE_MH, 0, 0).x);
  const bool acc = mh_accept<float>(t.H0[b], t.H1[b], t.lp1[b], u);
  const bool reset = (!acc) && (t.n == t.burn + 1);                  // SURVEY Q2 (samplers.py:1018)
  const int64_t e = b * D + j;
  if (j < D) {
    const float v = acc ? t.th[e] : (reset ? t.init[e] : t.cur[e]);
    t.cur[e] = v;
    if (t.row && t.n > t.burn) t.row[e] = v;
  }
  if (j == 0) {
    if (!acc) t.rej[b] += 1;
    if (t.acc) t.acc[b] = acc ? 1 : 0;
  }
}

}  // namespace hta
