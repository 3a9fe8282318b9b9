// What the chain-per-lane HMC skeletons share (hmc_callback.hip.in: one compiled callable; rolled_callback.hip.in: one rolled over its
// data rows; split_callback.hip.in: a list of them): the mass operations, the kinetic energy, the drift and the momentum draw of ONE
// chain held in a lane's registers, the body of hta_cb_predraw_kernel (the pre-drawn records of a launch), and for lists of
// callables subset_order, logp_total and the drift lengths.  The loop bodies the kernels share are text: cb_hmc_bodies.inc.
// Included AFTER "hta_cb_generated.inc" (which defines HTA_CB_D, HTA_CB_T and HTA_CB_MASS), cb_math.hpp and philox.hpp.
#ifndef HTA_CB_HMC_SHARED_HPP
#define HTA_CB_HMC_SHARED_HPP

namespace hta_cb {

typedef HTA_CB_T T;
constexpr int D = HTA_CB_D;
constexpr int NQ = (D + 3) / 4;

// v = M^-1 p   (samplers.py:283-296)
__device__ __forceinline__ void apply_inv_mass(const T (&p)[D], const T* __restrict__ im, T (&v)[D]) {
#if HTA_CB_MASS == 0
#pragma unroll
  for (int j = 0; j < D; ++j) v[j] = p[j];
#elif HTA_CB_MASS == 1
#pragma unroll
  for (int j = 0; j < D; ++j) v[j] = im[j] * p[j];
#else
#pragma unroll
  for (int j = 0; j < D; ++j) {
    T acc = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) acc += im[j * D + k] * p[k];
    v[j] = acc;
  }
#endif
}

__device__ __forceinline__ T kinetic(const T (&p)[D], const T* __restrict__ im) {
  T v[D];
  apply_inv_mass(p, im, v);
  T acc = 0;
#pragma unroll
  for (int j = 0; j < D; ++j) acc += p[j] * v[j];
  return (T)0.5 * acc;
}

__device__ __forceinline__ void drift(T (&th)[D], const T (&p)[D], const T* __restrict__ im, T eps) {
  T v[D];
  apply_inv_mass(p, im, v);
#pragma unroll
  for (int j = 0; j < D; ++j) th[j] += eps * v[j];
}

// p ~ N(0, M) from the (seed, chain, trajectory) Philox stream - the draw of hta_momentum_resample (csrc/hmc_pieces.hip)
__device__ __forceinline__ void draw_momentum(T (&p)[D], const T* __restrict__ mf, uint64_t seed, uint64_t chain, uint32_t n) {
  T z[4 * NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    T zz[4];
    hta::normal4<T>(hta::philox_block(seed, chain, n, hta::PURPOSE_MOMENTUM, 0, (uint32_t)q), zz);
#pragma unroll
    for (int i = 0; i < 4; ++i) z[4 * q + i] = zz[i];
  }
#if HTA_CB_MASS == 0
#pragma unroll
  for (int j = 0; j < D; ++j) p[j] = z[j];
#elif HTA_CB_MASS == 1
#pragma unroll
  for (int j = 0; j < D; ++j) p[j] = mf[j] * z[j];
#else
#pragma unroll
  for (int j = 0; j < D; ++j) {
    T acc = 0;
#pragma unroll
    for (int k = 0; k <= j; ++k) acc += mf[j * D + k] * z[k];
    p[j] = acc;
  }
#endif
}

// The draws of a launch's trajectories do not depend on the chains' states: with few chains (16 lone waves at 1024) they are 45 % of
// the trajectory kernel's instructions (Philox rounds, Box-Muller's log / sqrt / sincos) on its critical path.  hta_cb_predraw_kernel
// (blocks of 256 threads; HtaCbHmcArgs or HtaCbRolledArgs) produces them for the whole launch with the whole GPU - one thread per
// (trajectory, chain), records laid out [t][j][c] so that the consumer's loads are coalesced - and the trajectory kernel reads the
// next trajectory's record a trajectory ahead.  Same generator, same arithmetic: the results are bit-identical to the in-lane draw
// (tests/test_gpu_jit.py).
template <typename Args>
__device__ __forceinline__ void predraw_records(const Args& a) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= a.C * (int64_t)a.n_traj) return;
  const int t = (int)(id / a.C);
  const int64_t c = id - (int64_t)t * a.C;
  const uint64_t chain = a.chain_offset + (uint64_t)c;
  const uint32_t n = (uint32_t)(a.traj_offset + t);
  T p[D];
  draw_momentum(p, (const T*)a.mass_factor, a.seed, chain, n);
  T* __restrict__ rec = (T*)a.pre + (int64_t)t * (D + 1) * a.C + c;
#pragma unroll
  for (int j = 0; j < D; ++j) rec[(int64_t)j * a.C] = p[j];
  rec[(int64_t)D * a.C] = log(hta::u23<T>(hta::philox_block(a.seed, chain, n, hta::PURPOSE_MH, 0, 0).x));
}

#ifdef HTA_CB_M
// ---- lists of callables: the generated include defines HTA_CB_M, value_grad_m(m, th, lp, g) and value_m(m, th, lp) ----
constexpr int M = HTA_CB_M;
static_assert(M >= 1 && M <= HTA_CB_MAX_SPLIT, "a subset order packs into 16 four-bit fields");

// The order in which a trajectory (a leapfrog() call: n = 0, S:549) visits the subsets, four bits per position.  SPLITTING_RAND: hta::split_permutation - the integers
// of util.split_permutation and the oracle's philox_permutation (the reference: torch.randperm(M) once per leapfrog call, S:549).
// Packed so that the stage loop reads it with shifts of a scalar, not with a dynamic index into a private array.
__device__ __forceinline__ unsigned long long subset_order(int kind, uint64_t seed, uint32_t n) {
  unsigned long long order = 0xFEDCBA9876543210ull;
  if (kind == HTA_CB_SPLIT_RAND) {
    int perm[M];
    hta::split_permutation(seed, n, M, perm);
    order = 0;
#pragma unroll
    for (int i = 0; i < M; ++i) order |= (unsigned long long)(perm[i] & 15) << (4 * i);
  }
  return order;
}

// log p = sum over the subsets (S:787-796), in list order as _GenericHMC._logp adds them
__device__ __forceinline__ T logp_total(const T (&th)[D]) {
  T acc = 0;
#pragma nounroll
  for (int m = 0; m < M; ++m) {
    T v;
    value_m(m, th, v);
    acc += v;
  }
  return acc;
}

// the lengths as samplers._split_step hands them to hta_kick_drift: formed in double, rounded to T once
#define HTA_CB_SPLIT_LENGTHS(eps)                                                                                        \
  const T heps = (T)(0.5 * eps);                                                                                         \
  const T dr_sym = M > 1 ? (T)(eps / (double)((M - 1) * 2)) : (T)0; /* S:499-540: 2 (M - 1) drifts per step */           \
  const T dr_rand = (T)(eps / (double)M);                           /* S:547-566: M drifts per step         */           \
  const T dr_kmid = (T)eps;                                         /* S:572-596: one drift per step        */
#endif  // HTA_CB_M

}  // namespace hta_cb

// the sections of cb_hmc_bodies.inc
#define HTA_CB_BODY_TRAJECTORIES 1
#define HTA_CB_BODY_ACCEPT_TAIL 2
#define HTA_CB_BODY_LAUNCH_END 3
#define HTA_CB_BODY_SPLIT_STAGES 4

#endif
