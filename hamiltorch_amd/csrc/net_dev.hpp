// Small device helpers shared by the four deep-net sampler kernels (mlp_hmc_dev.hpp, mlp_mfma_dev.hpp, mlp3_mfma_dev.hpp,
// netn_hmc_dev.hpp): the activation and its derivative, the DPP getter, the sum over the 4 lane groups of a matrix-core tile.
#pragma once
#include "common.hpp"

namespace hta {

typedef float V4f __attribute__((ext_vector_type(4)));

template <int CTRL> __device__ __forceinline__ float dpp_get(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
// DPP controls: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_ror:4, row_ror:8
#define HTA_DPP_X1 0xB1
#define HTA_DPP_X2 0x4E
#define HTA_DPP_ROR4 0x124
#define HTA_DPP_ROR8 0x128

// sum over the 4 lane groups (g = lane >> 4); every lane gets the total
__device__ __forceinline__ float groups_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// activation (0 ReLU, 1 tanh, 2 sigmoid) from the pre-activation.  `act` is a template constant of the caller or a uniform
// run-time value (netn_hmc_dev.hpp): the function is inlined either way.  Three forms that differ in the ReLU only:
template <typename T> __device__ __forceinline__ T act_fn(int act, T z) {
  if (act == 0) return z > (T)0 ? z : (T)0;
  if (act == 1) return tanh(z);
  return (T)1 / ((T)1 + exp(-z));
}
// mlp_mfma_dev.hpp:
__device__ __forceinline__ float act_fn_med3(int act, float z) {
  // max(z, 0) in ONE VALU op, v_med3_f32(z, 0, FLT_MAX): fmaxf - and med3 against +inf, which the compiler folds into it -
  // compile to v_max(z, z) (a canonicalize) + v_max(0, .): 56 instead of 28 instructions per gradient at BASELINE config 4.
  // (An activation of +inf - a diverged chain - becomes FLT_MAX: the log-probability still overflows, the proposal is rejected.)
  if (act == 0) return __builtin_amdgcn_fmed3f(z, 0.0f, 3.4028234663852886e38f);
  return act_fn<float>(act, z);
}
// mlp3_mfma_dev.hpp: med3 against +inf, the form the compiler folds into fmaxf (see above); +inf stays +inf
__device__ __forceinline__ float act_fn_med3_inf(int act, float z) {
  if (act == 0) return __builtin_amdgcn_fmed3f(z, 0.0f, __builtin_inff());
  return act_fn<float>(act, z);
}
// the activation's derivative in terms of the activation VALUE
template <typename T> __device__ __forceinline__ T act_deriv(int act, T h) {
  if (act == 0) return h > (T)0 ? (T)1 : (T)0;
  if (act == 1) return (T)1 - h * h;
  return h * ((T)1 - h);
}

}  // namespace hta
