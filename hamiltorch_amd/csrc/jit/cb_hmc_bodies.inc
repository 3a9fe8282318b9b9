// The loop bodies the chain-per-lane kernels share, as TEXT: each section is included into the body of a kernel, which has defined the
// names the section uses.  Text and not functions, because the machine code must not move: the same statements inlined from a callee
// come out of the compiler with other registers and spills (profiles/r10a_jit_skeleton_isa.txt holds the kernels as they are).
//
//   #define HTA_CB_BODY HTA_CB_BODY_TRAJECTORIES | HTA_CB_BODY_ACCEPT_TAIL | HTA_CB_BODY_SPLIT_STAGES   (cb_hmc_shared.hpp)
//   #include "cb_hmc_bodies.inc"
//
// TRAJECTORIES (hta_cb_hmc_kernel, hta_cb_rolled_kernel): the reference's sample() loop for plain HMC (samplers.py:965-1026) for chain
//   `c` of the argument block `a`; `live`: this lane stores.  HTA_CB_EVAL(th, lp, g) is log p and its gradient at th, HTA_CB_BLOCK_SYNC
//   nothing where a lane is alone with its chain and `__syncthreads();` where several waves of a block run the same chains.
// ACCEPT_TAIL (TRAJECTORIES, hta_cb_split_kernel): the end of trajectory n - the Metropolis test on Ho, Hn, lp, logu, then accept / Q2
//   reset / restore on th (HTA_CB_CARRY_GRAD 1: and on g, through gcur), the rejection counter and the sample row.
// LAUNCH_END (the same two): the stores at the end of a launch.
// SPLIT_STAGES (hta_cb_split_kernel, hta_cb_split_path_kernel): n_stage stages of a split integrator on (th, p, g) under `kind`,
//   `order` and the lengths of HTA_CB_SPLIT_LENGTHS; HTA_CB_STEP_DONE is what follows a completed step (s2 == 0 again).
#if HTA_CB_BODY == HTA_CB_BODY_TRAJECTORIES
#undef HTA_CB_BODY
  T* __restrict__ cur = (T*)a.cur + c * D;
  T* __restrict__ gcur = (T*)a.gcur + c * D;
  const T* __restrict__ init = (const T*)a.init + c * D;
  const T* __restrict__ im = (const T*)a.inv_mass;
  const T* __restrict__ mf = (const T*)a.mass_factor;
  const T eps = (T)a.eps;
  const uint64_t chain = a.chain_offset + (uint64_t)c;

  T th[D], p[D], g[D];
#pragma unroll
  for (int j = 0; j < D; ++j) { th[j] = cur[j]; g[j] = 0; }
  // pre-drawn records (a.pre): the next trajectory's row is requested a trajectory ahead - one wait at its first use
  const T* __restrict__ pre = (const T*)a.pre;
  T rec[D + 1];
  if (pre && a.n_traj > 0) {
#pragma unroll
    for (int j = 0; j <= D; ++j) rec[j] = pre[(int64_t)j * a.C + c];
  }
  T lp_cur = 0;
  bool stale = true;             // this lane's (lp_cur, g) are not those of th
  if (a.resume) {                // a later launch of the same run: the carried pair is where the previous launch left it, bit for bit
    lp_cur = ((const T*)a.lp_out)[c];
#pragma unroll
    for (int j = 0; j < D; ++j) g[j] = gcur[j];
    stale = false;
  }
  int rejected = 0;
  T Ho = 0, Hn = 0;
  bool acc = false;

  for (int t = 0;; ++t) {
    const int n = a.traj_offset + t;
    // (log p, gradient) at the current point are CARRIED from trajectory to trajectory: the reference evaluates log p there for
    // H_old (samplers.py:971) and differentiates it again for the first half kick (samplers.py:281); both are known - the end of the
    // accepted proposal, or the start of the rejected one.  Evaluated afresh at the start of a run and after the Q2 reset (the
    // extra pass t == n_traj exists for a launch that ENDS with the Q2 trajectory: the workspace then holds the refreshed pair).
    if ((t == 0 && !a.resume) || (t > 0 && n - 1 == a.burn + 1)) {
      T lp2, g2[D];
      HTA_CB_EVAL(th, lp2, g2);
      if (stale) {
        lp_cur = lp2;
#pragma unroll
        for (int j = 0; j < D; ++j) { g[j] = g2[j]; if (live) gcur[j] = g2[j]; }
      }
      stale = false;
      HTA_CB_BLOCK_SYNC          // wave 0's store of gcur is in front of the other waves' read of it after a rejection in THIS
                                 // trajectory (L = 0 has no other barrier in between); block-uniform like the condition around it
    }
    if (t == a.n_traj) break;

    T logu = 0;
    if (pre) {
#pragma unroll
      for (int j = 0; j < D; ++j) p[j] = rec[j];
      logu = rec[D];
      if (t + 1 < a.n_traj) {
        const T* __restrict__ nx = pre + (int64_t)(t + 1) * (D + 1) * a.C + c;
#pragma unroll
        for (int j = 0; j <= D; ++j) rec[j] = nx[(int64_t)j * a.C];
      }
    } else {
      draw_momentum(p, mf, a.seed, chain, (uint32_t)n);                          // samplers.py:969
    }
    Ho = -lp_cur + kinetic(p, im);                                               // samplers.py:971
    T lp = lp_cur;
#pragma unroll
    for (int j = 0; j < D; ++j) p[j] += (T)0.5 * eps * g[j];                     // samplers.py:281
    for (int l = 0; l < a.L; ++l) {
      drift(th, p, im, eps);                                                     // samplers.py:284-296
      HTA_CB_EVAL(th, lp, g);                                                    // samplers.py:297
#pragma unroll
      for (int j = 0; j < D; ++j) p[j] += eps * g[j];                            // samplers.py:298
    }
#pragma unroll
    for (int j = 0; j < D; ++j) p[j] -= (T)0.5 * eps * g[j];                     // samplers.py:302
    Hn = -lp + kinetic(p, im);                                                   // samplers.py:995

    if (!pre) logu = log(hta::u23<T>(hta::philox_block(a.seed, chain, (uint32_t)n, hta::PURPOSE_MH, 0, 0).x));
#define HTA_CB_CARRY_GRAD 1
#define HTA_CB_BODY HTA_CB_BODY_ACCEPT_TAIL
#include "cb_hmc_bodies.inc"
    HTA_CB_BLOCK_SYNC            // wave 0's stores of (cur, gcur) are in front of every wave's reads of them in a later trajectory, and
                                 // this trajectory's reads are in front of its next stores
  }
#define HTA_CB_BODY HTA_CB_BODY_LAUNCH_END
#include "cb_hmc_bodies.inc"
#undef HTA_CB_CARRY_GRAD

#elif HTA_CB_BODY == HTA_CB_BODY_ACCEPT_TAIL
#undef HTA_CB_BODY
    acc = hta::finite_(Ho) && hta::finite_(Hn) && hta::finite_(lp) && (fmin((T)0, Ho - Hn) >= logu);   // samplers.py:1000-1004, :1045-1057 (mh_rules.hpp: mh_accept)
    rejected += acc ? 0 : 1;
    if (acc) {
      lp_cur = lp;
      if (live) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
        cur[j] = th[j];
#if HTA_CB_CARRY_GRAD
        gcur[j] = g[j];
#endif
      }
      }
    } else if (n == a.burn + 1) {                                                // SURVEY Q2 (samplers.py:1018): back to params_init
#pragma unroll
      for (int j = 0; j < D; ++j) { th[j] = init[j]; if (live) cur[j] = th[j]; }
      stale = true;
    } else {
#pragma unroll
      for (int j = 0; j < D; ++j) {
        th[j] = cur[j];
#if HTA_CB_CARRY_GRAD
        g[j] = gcur[j];
#endif
      }
    }
    if (n > a.burn && a.samples && live) {                                       // samplers.py:1008-1012, :1020-1024
      T* __restrict__ row = (T*)a.samples + ((int64_t)(n - a.burn) * a.C + c) * D;
#pragma unroll
      for (int j = 0; j < D; ++j) row[j] = th[j];
    }

#elif HTA_CB_BODY == HTA_CB_BODY_LAUNCH_END
#undef HTA_CB_BODY
  if (live) {
    a.reject_count[c] += rejected;
    if (a.H_old) ((T*)a.H_old)[c] = Ho;
    if (a.H_new) ((T*)a.H_new)[c] = Hn;
    if (a.accept) a.accept[c] = acc ? 1 : 0;
    if (a.lp_out) ((T*)a.lp_out)[c] = lp_cur;
  }

#elif HTA_CB_BODY == HTA_CB_BODY_SPLIT_STAGES
#undef HTA_CB_BODY
    // One stage = half kick by one subset's gradient + the drift that follows it (possibly none).  Position s2 = stage mod 2 M:
    //   symmetric  subsets 0 .. M-1, M-1 .. 0; a drift of eps / (2 (M-1)) after every kick but the turning point and the last
    //   rand       subsets order[0], order[0], order[1], order[1], ..; a drift of eps / M after the first kick of each pair
    //   kmid       subsets 0 .. M-1, M-1 .. 0; one drift of eps after kick M-1
    // A kick WITHOUT a drift is followed by a kick of the SAME subset at the same point (the turning point; the step boundary):
    // the gradient is evaluated once and applied twice - (2 M - 2) L + 1 evaluations per trajectory, as _split_step.  (The rand
    // scheme differentiates again after its drift-less kick only when M = 1; it does so here too: 2 M L.)
    int prev_m = -1, s2 = 0;
    bool prev_drifted = true;
#pragma nounroll
    for (int st = 0; st < n_stage; ++st) {
      int m;
      T dr;
      if (kind == HTA_CB_SPLIT_RAND) {
        m = (int)((order >> (4 * (s2 >> 1))) & 15ull);
        dr = (s2 & 1) ? (T)0 : dr_rand;
      } else {
        m = s2 < M ? s2 : 2 * M - 1 - s2;
        if (kind == HTA_CB_SPLIT_KMID) dr = s2 == M - 1 ? dr_kmid : (T)0;
        else dr = (s2 == M - 1 || s2 == 2 * M - 1) ? (T)0 : dr_sym;
      }
      const bool reuse = kind != HTA_CB_SPLIT_RAND && !prev_drifted && prev_m == m;
      if (!reuse) {
        T lp_unused;
        value_grad_m(m, th, lp_unused, g);                                       // the ONE call site of the subsets' gradients
      }
#pragma unroll
      for (int j = 0; j < D; ++j) p[j] += heps * g[j];
      const bool drifts = dr != (T)0;
      if (drifts) drift(th, p, im, dr);
      prev_m = m;
      prev_drifted = drifts;
      s2 = s2 + 1 == 2 * M ? 0 : s2 + 1;
      HTA_CB_STEP_DONE
    }

#else
#error "cb_hmc_bodies.inc: define HTA_CB_BODY"
#endif
