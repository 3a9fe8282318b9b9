// What the chain-per-lane HMC skeletons share (hmc_callback.hip.in: one compiled callable; split_callback.hip.in: a list of them):
// the mass operations, the kinetic energy, the drift and the momentum draw of ONE chain held in a lane's registers.
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

}  // namespace hta_cb

#endif
