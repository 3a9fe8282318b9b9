// Running moments of batched chains on the device: the per-chain mean and M2 (sum of squared deviations from the mean) of every
// coordinate of samples x[S, C, D], kept in fp64 in the caller's state[2][C][D] and updated chunk by chunk - the streaming half of
// diagnostics.hip (mean, sd, R-hat of runs that are never held in memory at once) and the statistic the cross-chain warm-up pools
// its diagonal mass from (hamiltorch_amd/adapt.py).
//
//   x        f32 or f64, unit stride in d, element strides for s and c passed in (the rules of hta_diag_*); converted on load, ALL
//            arithmetic in fp64
//   update   moments_update_kernel: a lane per series (c, d) - the flattened index c D + d is contiguous in a sample row, so a
//            wave reads a row coalesced -, a segment of R rows per blockIdx.y.  Welford's recurrence in row order (no sum of
//            squares: a series of mean 1e6 and sd 1 keeps its variance).  R = moments_segment_rows(S, C, D): 256, halved down to
//            32 while the grid is below MOM_TARGET_BLOCKS blocks (C D small against the machine).  One segment: the chunk is
//            merged into the state by the same lane (one launch, no workspace).  More: (mean, M2) per segment to the workspace,
//            moments_merge_kernel merges the segments in segment order and then the chunk into the state.
//   merge    Chan et al.: delta = m_b - m_a, mean = m_a + delta n_b / n, M2 = M2_a + M2_b + delta^2 n_a n_b / n.
//   finish   moments_finish_kernel: 16 coordinates x 16 chain slices per block; slice k sums the chains k, k + 16, ... in order,
//            the slices are added in order through LDS.  Two passes over the state: the sums, then the squared deviations of the
//            chain means from their mean.
//
// No floating-point atomics; the order of every sum depends on (S, C, D) alone, so equal inputs and equal chunking give equal
// bits, whatever the strides.  A non-finite draw (or an overflow) leaves NaN in the mean and M2 of its own (c, d) and nowhere else.
// Nothing here allocates or synchronises.
#include "common.hpp"
#include "moments_rows.hpp"

// every product and sum rounded on its own (the Makefile's -ffp-contract=on would fuse them): the recurrences below are then
// the IEEE operations of their restatement in tests/moments_cases.py, and the kernels are bound by their loads, not by these
#pragma clang fp contract(off)

namespace hta {

// MOM_THREADS, the segment constants and moments_segment_rows: moments_rows.hpp (shared with covariance.hip)
constexpr int MOM_FIN_D = 16, MOM_FIN_C = 16;

// Chan et al.: (na, ma, qa) <- (na, ma, qa) + (nb, mb, qb), nb > 0
__device__ __forceinline__ void mom_chan(double& na, double& ma, double& qa, double nb, double mb, double qb) {
  if (na == 0.0) { na = nb; ma = mb; qa = qb; return; }
  const double n = na + nb, dl = mb - ma;
  ma = ma + dl * (nb / n);
  qa = qa + qb + dl * dl * (na * nb / n);
  na = n;
}

__device__ __forceinline__ void mom_store(double* __restrict__ state, int64_t CD, int64_t j, double n_prev, double n, double m, double q) {
  double na = n_prev, ma = 0.0, qa = 0.0;
  if (n_prev > 0.0) { ma = state[j]; qa = state[CD + j]; }
  mom_chan(na, ma, qa, n, m, q);
  if (!(isfinite(ma) && isfinite(qa))) ma = qa = __builtin_nan("");
  state[j] = ma;
  state[CD + j] = qa;
}

template <typename T>
__global__ void __launch_bounds__(MOM_THREADS) moments_update_kernel(const T* __restrict__ x, int64_t ss, int64_t sc, int64_t S, int64_t C, int64_t D, int64_t R,
                                                                     double n_prev, double* __restrict__ state, double* __restrict__ part) {
  const int64_t j = blockIdx.x * (int64_t)MOM_THREADS + threadIdx.x, CD = C * D;
  if (j >= CD) return;
  const int64_t c = j / D, d = j - c * D;
  const int64_t r0 = (int64_t)blockIdx.y * R, r1 = r0 + R < S ? r0 + R : S;
  const T* xs = x + c * sc + d;
  double m = 0.0, q = 0.0, k = 0.0;
  constexpr int U = 4;                                            // rows in flight per batch of loads
  int64_t s = r0;
  for (; s + U <= r1; s += U) {
    T v[U];
#pragma unroll
    for (int i = 0; i < U; ++i) v[i] = xs[(s + i) * ss];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      k += 1.0;
      const double dl = (double)v[i] - m;
      m = m + dl / k;
      q = q + dl * ((double)v[i] - m);
    }
  }
  for (; s < r1; ++s) {
    const double v = (double)xs[s * ss];
    k += 1.0;
    const double dl = v - m;
    m = m + dl / k;
    q = q + dl * (v - m);
  }
  if (gridDim.y == 1) {
    mom_store(state, CD, j, n_prev, k, m, q);
  } else {
    double* out = part + (int64_t)blockIdx.y * 2 * CD + j;
    out[0] = m;
    out[CD] = q;
  }
}

__global__ void __launch_bounds__(MOM_THREADS) moments_merge_kernel(const double* __restrict__ part, int64_t S, int64_t CD, int64_t R, int64_t nseg, double n_prev,
                                                                    double* __restrict__ state) {
  const int64_t j = blockIdx.x * (int64_t)MOM_THREADS + threadIdx.x;
  if (j >= CD) return;
  double n = 0.0, m = 0.0, q = 0.0;
  for (int64_t g = 0; g < nseg; ++g) {
    const int64_t r0 = g * R, r1 = r0 + R < S ? r0 + R : S;
    mom_chan(n, m, q, (double)(r1 - r0), part[g * 2 * CD + j], part[g * 2 * CD + CD + j]);
  }
  mom_store(state, CD, j, n_prev, n, m, q);
}

// sums of a[k][dx] over the chain slices k in order, to every thread of the column
__device__ __forceinline__ double mom_slices(double (&red)[MOM_FIN_C][MOM_FIN_D + 1], int cy, int dx, double a) {
  __syncthreads();
  red[cy][dx] = a;
  __syncthreads();
  double s = red[0][dx];
#pragma unroll
  for (int i = 1; i < MOM_FIN_C; ++i) s += red[i][dx];
  return s;
}

__global__ void __launch_bounds__(MOM_THREADS) moments_finish_kernel(const double* __restrict__ state, int64_t C, int64_t D, double n, double* __restrict__ mean_out,
                                                                     double* __restrict__ vw_out, double* __restrict__ vb_out, double* __restrict__ vt_out,
                                                                     double* __restrict__ rhat_out, double reg_n, double reg_floor, float* __restrict__ im32,
                                                                     double* __restrict__ im64) {
  __shared__ double red[MOM_FIN_C][MOM_FIN_D + 1];
  const int dx = threadIdx.x & (MOM_FIN_D - 1), cy = threadIdx.x / MOM_FIN_D;
  const int64_t d = blockIdx.x * (int64_t)MOM_FIN_D + dx, CD = C * D;
  const bool live = d < D;
  double a = 0.0, b = 0.0;
  if (live)
    for (int64_t c = cy; c < C; c += MOM_FIN_C) { a += state[c * D + d]; b += state[CD + c * D + d]; }
  const double nc = (double)C;
  const double mean = mom_slices(red, cy, dx, a) / nc;
  const double m2 = mom_slices(red, cy, dx, b);
  double e = 0.0;
  if (live)
    for (int64_t c = cy; c < C; c += MOM_FIN_C) { const double dm = state[c * D + d] - mean; e += dm * dm; }
  const double ssb = mom_slices(red, cy, dx, e);
  if (!live || cy != 0) return;
  const double vw = m2 / (n - 1.0) / nc;
  const double vb = C > 1 ? ssb / (nc - 1.0) : 0.0;
  const double N = n * nc;
  const double vt = (m2 + n * ssb) / (N - 1.0);
  if (mean_out) mean_out[d] = mean;
  if (vw_out) vw_out[d] = vw;
  if (vb_out) vb_out[d] = vb;
  if (vt_out) vt_out[d] = vt;
  if (rhat_out) {
    double rh = __builtin_nan("");                               // ess.py: rhat_split on the unsplit chains
    if (n >= 2.0) {
      if (vw <= 0.0) rh = vb > 0.0 ? __builtin_inf() : __builtin_nan("");
      else rh = sqrt(((n - 1.0) / n * vw + vb) / vw);
    }
    rhat_out[d] = rh;
  }
  if (im32 || im64) {
    const double im = vt * (N / (N + reg_n)) + reg_floor * (reg_n / (N + reg_n));
    if (im32) im32[d] = (float)im;
    if (im64) im64[d] = im;
  }
}

static int moments_check(const char* who, int64_t S, int64_t C, int64_t D) {
  HTA_REQUIRE(S >= 1 && C >= 1 && D >= 1 && S < (1ll << 31) && D < (1ll << 31) && C < (1ll << 31) && C * D < (1ll << 38), "%s: bad shape (S=%lld C=%lld D=%lld)", who,
              (long long)S, (long long)C, (long long)D);
  return HTA_OK;
}

template <typename T>
static int moments_update(const T* x, int64_t ss, int64_t sc, int64_t S, int64_t C, int64_t D, int64_t n_prev, double* state, void* workspace, int64_t workspace_bytes,
                          void* stream) {
  const char* who = "hta_moments_update";
  if (int rc = moments_check(who, S, C, D)) return rc;
  HTA_REQUIRE(x && state, "%s: x or state is NULL", who);
  HTA_REQUIRE(((uintptr_t)state & 7) == 0, "%s: state must be 8-byte aligned", who);
  HTA_REQUIRE(n_prev >= 0 && n_prev < (1ll << 52), "%s: n_prev=%lld", who, (long long)n_prev);
  HTA_REQUIRE(sc >= D && ss >= (C - 1) * sc + D, "%s: bad strides (stride_s=%lld stride_c=%lld): rows and chains must not overlap", who, (long long)ss, (long long)sc);
  const int64_t R = moments_segment_rows(S, C, D), nseg = (S + R - 1) / R, CD = C * D;
  HTA_REQUIRE(nseg <= 65535, "%s: S=%lld is beyond 65535 segments of %lld rows", who, (long long)S, (long long)R);
  const int64_t need = nseg > 1 ? 16 * nseg * CD : 0;
  HTA_REQUIRE(need == 0 || (workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= need), "%s: workspace of %lld bytes (8-byte aligned) needed, %lld given", who,
              (long long)need, (long long)workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  const unsigned bx = (unsigned)((CD + MOM_THREADS - 1) / MOM_THREADS);
  note_route("moments_update_kernel<%s>", sizeof(T) == 4 ? "float" : "double");
  moments_update_kernel<T><<<dim3(bx, (unsigned)nseg), MOM_THREADS, 0, st>>>(x, ss, sc, S, C, D, R, (double)n_prev, state, (double*)workspace);
  HTA_CHECK_LAUNCH("moments_update_kernel");
  if (nseg > 1) {
    moments_merge_kernel<<<bx, MOM_THREADS, 0, st>>>((const double*)workspace, S, CD, R, nseg, (double)n_prev, state);
    HTA_CHECK_LAUNCH("moments_merge_kernel");
  }
  return HTA_OK;
}

}  // namespace hta

extern "C" {

int64_t hta_moments_workspace_bytes(int64_t S, int64_t C, int64_t D) {
  if (S < 1 || C < 1 || D < 1 || S >= (1ll << 31) || C >= (1ll << 31) || D >= (1ll << 31)) return -1;
  const int64_t R = hta::moments_segment_rows(S, C, D), nseg = (S + R - 1) / R;
  return nseg > 1 ? 16 * nseg * C * D : 0;
}

int hta_moments_update_f32(const float* x, int64_t stride_s, int64_t stride_c, int64_t S, int64_t C, int64_t D, int64_t n_prev, double* state, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  return hta::moments_update<float>(x, stride_s, stride_c, S, C, D, n_prev, state, workspace, workspace_bytes, stream);
}
int hta_moments_update_f64(const double* x, int64_t stride_s, int64_t stride_c, int64_t S, int64_t C, int64_t D, int64_t n_prev, double* state, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  return hta::moments_update<double>(x, stride_s, stride_c, S, C, D, n_prev, state, workspace, workspace_bytes, stream);
}

int hta_moments_finish(int64_t C, int64_t D, int64_t n, const double* state, double* mean, double* var_within, double* var_between, double* var_total, double* rhat,
                       double reg_n, double reg_floor, float* inv_mass_f32, double* inv_mass_f64, void* stream) {
  using namespace hta;
  if (int rc = moments_check("hta_moments_finish", 1, C, D)) return rc;
  HTA_REQUIRE(n >= 1 && n < (1ll << 52), "hta_moments_finish: n=%lld draws", (long long)n);
  HTA_REQUIRE(state, "hta_moments_finish: state is NULL");
  HTA_REQUIRE(!(inv_mass_f32 || inv_mass_f64) || (reg_n >= 0.0 && reg_floor >= 0.0), "hta_moments_finish: bad regularisation (reg_n=%g reg_floor=%g)", reg_n, reg_floor);
  moments_finish_kernel<<<(unsigned)((D + MOM_FIN_D - 1) / MOM_FIN_D), MOM_THREADS, 0, (hipStream_t)stream>>>(state, C, D, (double)n, mean, var_within, var_between, var_total,
                                                                                                          rhat, reg_n, reg_floor, inv_mass_f32, inv_mass_f64);
  HTA_CHECK_LAUNCH("moments_finish_kernel");
  return HTA_OK;
}

}  // extern "C"
