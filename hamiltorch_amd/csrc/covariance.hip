// Running covariance of batched chains on the device: the per-chain means and the upper triangle of the co-moments
// q_ij = sum_s (x_si - m_i)(x_sj - m_j) of samples x[S, C, D], kept in fp64 in the caller's state and updated chunk by chunk - the
// matrix counterpart of moments.hip and the statistic the cross-chain warm-up pools its dense mass from (hamiltorch_amd/adapt.py).
//
//   state    mean[C][D] followed by comoment[C][T], T = D (D + 1) / 2: the pairs i <= j packed row-major.  The row count n is the
//            caller's.
//   x        f32 or f64, unit stride in d, element strides for s and c passed in; converted on load, ALL arithmetic in fp64
//   update   cov_update_kernel: a lane per (chain, pair) - the flattened index c T + t is contiguous in the state -, a segment of
//            R = moments_segment_rows(S, C, D) rows per blockIdx.y.  A workgroup owns WHOLE chains: 256 / T of them where T is
//            small, else one chain whose pairs the lanes walk 256 at a time.  Per row, in row order, for the pair (i, j):
//              k += 1; di = x_i - m_i; dj = x_j - m_j; m_i += di / k; m_j += dj / k; q += di (x_j - m_j)
//            - every lane carries its two means itself, so their bits do not depend on the pair, and on the diagonal this is the
//            Welford recurrence of moments_update_kernel.  One segment: the chunk is merged into the state by the same lane (one
//            launch, no workspace).  More: (mean, q) per segment to the workspace, cov_merge_kernel merges the segments in
//            segment order and then the chunk into the state.
//   merge    Chan et al. per pair: q = q_a + q_b + di dj n_a n_b / n with di = m_b,i - m_a,i, the means as in mom_chan.
//   owning   the merge into the state reads the old means of BOTH coordinates of a pair and the diagonal lanes write the new
//            ones: the workgroup copies its chains' old means to LDS before any lane writes, and no other workgroup touches them.
//   finish   cov_finish_kernel: 16 pairs x 16 chain slices per block; slice k sums the chains k, k + 16, ... in order, the slices
//            are added in order through LDS (the sums of moments_finish_kernel, so the diagonal and R-hat are its bits).
//
// No floating-point atomics; the order of every sum depends on (S, C, D) alone, so equal inputs and equal chunking give equal
// bits, whatever the strides.  A non-finite draw at (c, d) leaves NaN in mean[c][d] and in every co-moment of chain c that involves
// d, and nowhere else.  Nothing here allocates or synchronises.
#include "common.hpp"
#include "moments_rows.hpp"

// every product and sum rounded on its own: the recurrences below are the IEEE operations of tests/cov_cases.py
#pragma clang fp contract(off)

namespace hta {

constexpr int COV_THREADS = 256;
constexpr int COV_MAX_D = HTA_COV_MAX_D;
constexpr int COV_FIN_P = 16, COV_FIN_C = 16;
static_assert(COV_FIN_C == 16, "the chain slices of moments_finish_kernel");

static inline int64_t cov_pairs(int64_t D) { return D * (D + 1) / 2; }
// whole chains per workgroup of the update and merge kernels
static inline int64_t cov_chains_per_block(int64_t D) {
  const int64_t T = cov_pairs(D);
  return T >= COV_THREADS ? 1 : COV_THREADS / T;
}

// the pair t of the packed triangle -> row i and offset r = j - i (row i holds D - i pairs)
__device__ __forceinline__ void cov_pair(int64_t t, int D, int& i, int& r) {
  i = 0;
  while (t >= D - i) { t -= D - i; ++i; }
  r = (int)t;
}

// Chan et al. for one pair: (na, mai, maj, qa) <- (na, mai, maj, qa) + (nb, mbi, mbj, qb), nb > 0
__device__ __forceinline__ void cov_chan(double& na, double& mai, double& maj, double& qa, double nb, double mbi, double mbj, double qb) {
  if (na == 0.0) { na = nb; mai = mbi; maj = mbj; qa = qb; return; }
  const double n = na + nb, di = mbi - mai, dj = mbj - maj;
  mai = mai + di * (nb / n);
  maj = maj + dj * (nb / n);
  qa = qa + qb + di * dj * (na * nb / n);
  na = n;
}

// the chunk (n, mi, mj, q) of pair (i, j = i + r) of chain c into the state; old[] = the old means of the workgroup's chains
__device__ __forceinline__ void cov_store(double* __restrict__ state, const double* old, int64_t CD, int64_t T, int64_t D, int64_t c, int cl, int64_t t, int i,
                                          int r, double n_prev, double n, double mi, double mj, double q) {
  double na = n_prev, mai = 0.0, maj = 0.0, qa = 0.0;
  if (n_prev > 0.0) { mai = old[cl * D + i]; maj = old[cl * D + i + r]; qa = state[CD + c * T + t]; }
  cov_chan(na, mai, maj, qa, n, mi, mj, q);
  if (!(isfinite(mai) && isfinite(maj) && isfinite(qa))) qa = __builtin_nan("");
  state[CD + c * T + t] = qa;
  if (r == 0) state[c * D + i] = isfinite(qa) ? mai : __builtin_nan("");
}

__device__ __forceinline__ void cov_stage_means(double* old, const double* __restrict__ state, int64_t D, int64_t c0, int nch, double n_prev) {
  if (n_prev > 0.0)
    for (int k = threadIdx.x; k < nch * D; k += COV_THREADS) old[k] = state[c0 * D + k];
  __syncthreads();
}

template <typename T_>
__global__ void __launch_bounds__(COV_THREADS) cov_update_kernel(const T_* __restrict__ x, int64_t ss, int64_t sc, int64_t S, int64_t C, int D, int64_t R, int cpb,
                                                                 double n_prev, double* __restrict__ state, double* __restrict__ part) {
  __shared__ double old[COV_MAX_D];                               // cpb D <= 256: cpb = 256 / T chains where T < 256, else one
  const int64_t T = (int64_t)D * (D + 1) / 2, CD = C * D;
  const int64_t c0 = (int64_t)blockIdx.x * cpb;
  const int nch = (int)(C - c0 < cpb ? C - c0 : cpb);
  const bool direct = gridDim.y == 1;
  cov_stage_means(old, state, D, c0, nch, direct ? n_prev : 0.0);
  const int64_t r0 = (int64_t)blockIdx.y * R, r1 = r0 + R < S ? r0 + R : S;
  const int64_t work = nch * T;                                   // more than 256 only where the workgroup owns one chain
  int64_t w = threadIdx.x;
  if (w >= work) return;
  const int cl = (int)(w / T);
  int64_t t = w - cl * T;
  const int64_t c = c0 + cl;
  int i, r;
  cov_pair(t, D, i, r);
  for (;;) {
    const T_* xi = x + c * sc + i;
    const T_* xj = xi + r;
    double mi = 0.0, mj = 0.0, q = 0.0, k = 0.0;
    constexpr int U = 4;                                          // rows in flight per batch of loads
    int64_t s = r0;
    for (; s + U <= r1; s += U) {
      T_ vi[U], vj[U];
#pragma unroll
      for (int u = 0; u < U; ++u) { vi[u] = xi[(s + u) * ss]; vj[u] = xj[(s + u) * ss]; }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        k += 1.0;
        const double di = (double)vi[u] - mi, dj = (double)vj[u] - mj;
        mi = mi + di / k;
        mj = mj + dj / k;
        q = q + di * ((double)vj[u] - mj);
      }
    }
    for (; s < r1; ++s) {
      const double vi = (double)xi[s * ss], vj = (double)xj[s * ss];
      k += 1.0;
      const double di = vi - mi, dj = vj - mj;
      mi = mi + di / k;
      mj = mj + dj / k;
      q = q + di * (vj - mj);
    }
    if (direct) {
      cov_store(state, old, CD, T, D, c, cl, t, i, r, n_prev, k, mi, mj, q);
    } else {
      double* out = part + (int64_t)blockIdx.y * (CD + C * T);
      out[CD + c * T + t] = q;
      if (r == 0) out[c * D + i] = mi;
    }
    t += COV_THREADS;                                             // the next pair of this lane (one chain per workgroup)
    if (t >= work) break;
    r += COV_THREADS;
    while (r >= D - i) { r -= D - i; ++i; }
  }
}

__global__ void __launch_bounds__(COV_THREADS) cov_merge_kernel(const double* __restrict__ part, int64_t S, int64_t C, int D, int64_t R, int64_t nseg, int cpb,
                                                                double n_prev, double* __restrict__ state) {
  __shared__ double old[COV_MAX_D];
  const int64_t T = (int64_t)D * (D + 1) / 2, CD = C * D, seg = CD + C * T;
  const int64_t c0 = (int64_t)blockIdx.x * cpb;
  const int nch = (int)(C - c0 < cpb ? C - c0 : cpb);
  cov_stage_means(old, state, D, c0, nch, n_prev);
  const int64_t work = nch * T;
  int64_t w = threadIdx.x;
  if (w >= work) return;
  const int cl = (int)(w / T);
  int64_t t = w - cl * T;
  const int64_t c = c0 + cl;
  int i, r;
  cov_pair(t, D, i, r);
  for (;;) {
    double n = 0.0, mi = 0.0, mj = 0.0, q = 0.0;
    for (int64_t g = 0; g < nseg; ++g) {
      const int64_t r0 = g * R, r1 = r0 + R < S ? r0 + R : S;
      const double* p = part + g * seg;
      cov_chan(n, mi, mj, q, (double)(r1 - r0), p[c * D + i], p[c * D + i + r], p[CD + c * T + t]);
    }
    cov_store(state, old, CD, T, D, c, cl, t, i, r, n_prev, n, mi, mj, q);
    t += COV_THREADS;
    if (t >= work) break;
    r += COV_THREADS;
    while (r >= D - i) { r -= D - i; ++i; }
  }
}

// sums of a[k][px] over the chain slices k in order, to every thread of the column (mom_slices of moments.hip)
__device__ __forceinline__ double cov_slices(double (&red)[COV_FIN_C][COV_FIN_P + 1], int cy, int px, double a) {
  __syncthreads();
  red[cy][px] = a;
  __syncthreads();
  double s = red[0][px];
#pragma unroll
  for (int k = 1; k < COV_FIN_C; ++k) s += red[k][px];
  return s;
}

__global__ void __launch_bounds__(COV_THREADS) cov_finish_kernel(const double* __restrict__ state, int64_t C, int D, double n, double* __restrict__ mean_out,
                                                                 double* __restrict__ cw_out, double* __restrict__ ct_out, double* __restrict__ rhat_out, double reg_n,
                                                                 double reg_floor, float* __restrict__ im32, double* __restrict__ im64) {
  __shared__ double red[COV_FIN_C][COV_FIN_P + 1];
  const int px = threadIdx.x & (COV_FIN_P - 1), cy = threadIdx.x / COV_FIN_P;
  const int64_t T = (int64_t)D * (D + 1) / 2, CD = C * D;
  const int64_t t = blockIdx.x * (int64_t)COV_FIN_P + px;
  const bool live = t < T;
  int i = 0, r = 0;
  if (live) cov_pair(t, D, i, r);
  const int j = i + r;
  double ai = 0.0, aj = 0.0, b = 0.0;
  if (live)
    for (int64_t c = cy; c < C; c += COV_FIN_C) { ai += state[c * D + i]; aj += state[c * D + j]; b += state[CD + c * T + t]; }
  const double nc = (double)C;
  const double mean_i = cov_slices(red, cy, px, ai) / nc;
  const double mean_j = cov_slices(red, cy, px, aj) / nc;
  const double m2 = cov_slices(red, cy, px, b);
  double e = 0.0;
  if (live)
    for (int64_t c = cy; c < C; c += COV_FIN_C) { const double dmi = state[c * D + i] - mean_i, dmj = state[c * D + j] - mean_j; e += dmi * dmj; }
  const double ssb = cov_slices(red, cy, px, e);
  if (!live || cy != 0) return;
  const double cw = m2 / (n - 1.0) / nc;
  const double N = n * nc;
  const double ct = (m2 + n * ssb) / (N - 1.0);
  const int64_t ij = (int64_t)i * D + j, ji = (int64_t)j * D + i;
  if (cw_out) cw_out[ij] = cw_out[ji] = cw;
  if (ct_out) ct_out[ij] = ct_out[ji] = ct;
  if (im32 || im64) {
    double im = ct * (N / (N + reg_n));
    if (r == 0) im = im + reg_floor * (reg_n / (N + reg_n));
    if (im32) im32[ij] = im32[ji] = (float)im;
    if (im64) im64[ij] = im64[ji] = im;
  }
  if (r != 0) return;
  if (mean_out) mean_out[i] = mean_i;
  if (rhat_out) {
    const double vb = C > 1 ? ssb / (nc - 1.0) : 0.0;
    double rh = __builtin_nan("");                               // moments_finish_kernel's R-hat of the unsplit chains
    if (n >= 2.0) {
      if (cw <= 0.0) rh = vb > 0.0 ? __builtin_inf() : __builtin_nan("");
      else rh = sqrt(((n - 1.0) / n * cw + vb) / cw);
    }
    rhat_out[i] = rh;
  }
}

static int cov_check(const char* who, int64_t S, int64_t C, int64_t D) {
  HTA_REQUIRE(S >= 1 && C >= 1 && D >= 1 && S < (1ll << 31) && D < (1ll << 31) && C < (1ll << 31), "%s: bad shape (S=%lld C=%lld D=%lld)", who, (long long)S,
              (long long)C, (long long)D);
  HTA_REQUIRE(D <= COV_MAX_D, "%s: D=%lld is beyond the limit of %d coordinates (HTA_COV_MAX_D)", who, (long long)D, COV_MAX_D);
  return HTA_OK;
}

template <typename T_>
static int cov_update(const T_* x, int64_t ss, int64_t sc, int64_t S, int64_t C, int64_t D, int64_t n_prev, double* state, void* workspace, int64_t workspace_bytes,
                      void* stream) {
  const char* who = "hta_cov_update";
  if (int rc = cov_check(who, S, C, D)) return rc;
  HTA_REQUIRE(x && state, "%s: x or state is NULL", who);
  HTA_REQUIRE(((uintptr_t)state & 7) == 0, "%s: state must be 8-byte aligned", who);
  HTA_REQUIRE(n_prev >= 0 && n_prev < (1ll << 52), "%s: n_prev=%lld", who, (long long)n_prev);
  HTA_REQUIRE(sc >= D && ss >= (C - 1) * sc + D, "%s: bad strides (stride_s=%lld stride_c=%lld): rows and chains must not overlap", who, (long long)ss, (long long)sc);
  const int64_t R = moments_segment_rows(S, C, D), nseg = (S + R - 1) / R, T = cov_pairs(D);
  HTA_REQUIRE(nseg <= 65535, "%s: S=%lld is beyond 65535 segments of %lld rows", who, (long long)S, (long long)R);
  const int64_t need = nseg > 1 ? 8 * nseg * C * (D + T) : 0;
  HTA_REQUIRE(need == 0 || (workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= need), "%s: workspace of %lld bytes (8-byte aligned) needed, %lld given", who,
              (long long)need, (long long)workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  const int64_t cpb = cov_chains_per_block(D);
  const unsigned bx = (unsigned)((C + cpb - 1) / cpb);
  note_route("cov_update_kernel<%s>", sizeof(T_) == 4 ? "float" : "double");
  cov_update_kernel<T_><<<dim3(bx, (unsigned)nseg), COV_THREADS, 0, st>>>(x, ss, sc, S, C, (int)D, R, (int)cpb, (double)n_prev, state, (double*)workspace);
  HTA_CHECK_LAUNCH("cov_update_kernel");
  if (nseg > 1) {
    cov_merge_kernel<<<bx, COV_THREADS, 0, st>>>((const double*)workspace, S, C, (int)D, R, nseg, (int)cpb, (double)n_prev, state);
    HTA_CHECK_LAUNCH("cov_merge_kernel");
  }
  return HTA_OK;
}

}  // namespace hta

extern "C" {

int64_t hta_cov_workspace_bytes(int64_t S, int64_t C, int64_t D) {
  if (S < 1 || C < 1 || D < 1 || S >= (1ll << 31) || C >= (1ll << 31) || D > HTA_COV_MAX_D) return -1;
  const int64_t R = hta::moments_segment_rows(S, C, D), nseg = (S + R - 1) / R;
  return nseg > 1 ? 8 * nseg * C * (D + hta::cov_pairs(D)) : 0;
}

int64_t hta_cov_state_bytes(int64_t C, int64_t D) {
  if (C < 1 || D < 1 || C >= (1ll << 31) || D > HTA_COV_MAX_D) return -1;
  return 8 * C * (D + hta::cov_pairs(D));
}

int hta_cov_update_f32(const float* x, int64_t stride_s, int64_t stride_c, int64_t S, int64_t C, int64_t D, int64_t n_prev, double* state, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  return hta::cov_update<float>(x, stride_s, stride_c, S, C, D, n_prev, state, workspace, workspace_bytes, stream);
}
int hta_cov_update_f64(const double* x, int64_t stride_s, int64_t stride_c, int64_t S, int64_t C, int64_t D, int64_t n_prev, double* state, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  return hta::cov_update<double>(x, stride_s, stride_c, S, C, D, n_prev, state, workspace, workspace_bytes, stream);
}

int hta_cov_finish(int64_t C, int64_t D, int64_t n, const double* state, double* mean, double* cov_within, double* cov_total, double* rhat, double reg_n,
                   double reg_floor, float* inv_mass_f32, double* inv_mass_f64, void* stream) {
  using namespace hta;
  if (int rc = cov_check("hta_cov_finish", 1, C, D)) return rc;
  HTA_REQUIRE(n >= 1 && n < (1ll << 52), "hta_cov_finish: n=%lld draws", (long long)n);
  HTA_REQUIRE(state, "hta_cov_finish: state is NULL");
  HTA_REQUIRE(((uintptr_t)state & 7) == 0, "hta_cov_finish: state must be 8-byte aligned");
  HTA_REQUIRE(!(inv_mass_f32 || inv_mass_f64) || (reg_n >= 0.0 && reg_floor >= 0.0), "hta_cov_finish: bad regularisation (reg_n=%g reg_floor=%g)", reg_n, reg_floor);
  const int64_t T = cov_pairs(D);
  cov_finish_kernel<<<(unsigned)((T + COV_FIN_P - 1) / COV_FIN_P), COV_THREADS, 0, (hipStream_t)stream>>>(state, C, (int)D, (double)n, mean, cov_within, cov_total, rhat, reg_n,
                                                                                                       reg_floor, inv_mass_f32, inv_mass_f64);
  HTA_CHECK_LAUNCH("cov_finish_kernel");
  return HTA_OK;
}

}  // extern "C"
