// Convergence diagnostics of batched chains on the device: bulk ESS (linear autocovariance with divisor S, Geyer's initial
// positive sequence, multi-chain variance as in Vehtari et al. 2021 without rank-normalisation) and split R-hat - the definitions
// of hamiltorch_amd/ess.py, for every coordinate of samples x[S, C, D] at once.
//
//   x        f32 or f64, unit stride in d, element strides for s and c passed in (a row offset or a leading-coordinate slice of
//            a sample buffer is read in place); converted on load, ALL arithmetic in fp64
//   moments  diag_moments_kernel: a lane per series (c, d) - the flattened index c D + d is contiguous in a sample row -, a
//            segment of DIAG_SEGMENT_ROWS rows per blockIdx.y.  Per segment and series the mean and M2 of its rows of the first
//            and of the last S/2 rows, as deviations from the first such row (no plain sum of squares).
//            diag_combine_kernel: a block per coordinate; per chain the segments merged in order with Chan's pairwise formula
//            (halves -> whole chain), then the sums over chains (deviations from chain 0's values) through an LDS tree.
//   lags     diag_lags_kernel<T, B>: a block of B consecutive lags per blockIdx.z.  A lane owns coordinate d of the chains
//            cg, cg + G, ... (G = min(C, DIAG_CHAIN_GROUPS)); walking the rows of its segment it keeps the last B centred values of the
//            lagged stream in registers and adds B products per row, so x is read once per block of lags and not once per lag.
//            diag_lag_reduce_kernel sums the (segment, chain group) partials in a fixed order into acov[t, d].
//   finish   diag_finish_kernel: per coordinate the Geyer walk resumed over the lags of this call, (tau, t, done) kept in device
//            memory, and the number of coordinates not yet done counted into one int32 (an integer atomic per block).
//
// No floating-point atomics: partial results go to the caller's workspace and are combined in an order that depends on (S, C)
// alone - not on D, strides or the coordinate chunking -, so equal inputs give equal bits.  Nothing here allocates or synchronises.
#include "common.hpp"

namespace hta {

constexpr int DIAG_LAG_BLOCK = 16;        // B: lags per lag block (16 sums + 16 window values in fp64 = 64 of the kernel's <= 128 registers)
constexpr int DIAG_SEGMENT_ROWS = 256;    // R: rows of S per segment (blockIdx.y)
constexpr int DIAG_CHAIN_GROUPS = 1024;   // G <= this: chains c, c + G, ... share a lane of the lag kernel
constexpr int DIAG_MAX_LAG_BLOCKS = 32;   // lag blocks per launch (blockIdx.z)
constexpr int DIAG_THREADS = 256;

struct DiagLayout {           // workspace, in 8-byte words
  int64_t nseg, G, P;         // segments of S, chain groups, partial rows per lag (nseg * G)
  int64_t mean_var, var_plus, tau, t, done, series_mean, mom, acov, total_fixed;
};

static DiagLayout diag_layout(int64_t S, int64_t C, int64_t D) {
  DiagLayout L;
  L.nseg = (S + DIAG_SEGMENT_ROWS - 1) / DIAG_SEGMENT_ROWS;
  L.G = C < DIAG_CHAIN_GROUPS ? C : DIAG_CHAIN_GROUPS;
  L.P = L.nseg * L.G;
  const int64_t half = (D + 1) / 2;
  L.mean_var = 0;
  L.var_plus = L.mean_var + D;
  L.tau = L.var_plus + D;
  L.t = L.tau + D;
  L.done = L.t + half;
  L.series_mean = L.done + half;
  L.mom = L.series_mean + C * D;
  L.acov = L.mom + 4 * L.nseg * C * D;
  L.total_fixed = L.acov;
  return L;
}
static int64_t diag_words(const DiagLayout& L, int64_t D, int64_t n_lags) { return L.total_fixed + n_lags * D + n_lags * L.P * D; }

// (n, mean, M2) of rows [a, b) of one series as deviations from row a
template <typename T>
__device__ __forceinline__ void diag_rows(const T* __restrict__ xs, int64_t ss, int64_t a, int64_t b, double& mean, double& m2) {
  mean = 0.0; m2 = 0.0;
  if (b <= a) return;
  const double shift = (double)xs[a * ss];
  double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
  for (int64_t s = a + 1; s < b; ++s) {
    const double d = (double)xs[s * ss] - shift;
    s1 += d;
    s2 += d * d;
  }
  const double n = (double)(b - a);
  mean = shift + s1 / n;
  m2 = s2 - s1 * s1 / n;
  if (m2 < 0.0) m2 = 0.0;
}

// Chan et al.: (na, ma, qa) <- (na, ma, qa) + (nb, mb, qb)
__device__ __forceinline__ void diag_chan(double& na, double& ma, double& qa, double nb, double mb, double qb) {
  if (nb == 0.0) return;
  if (na == 0.0) { na = nb; ma = mb; qa = qb; return; }
  const double n = na + nb, dl = mb - ma;
  qa = qa + qb + dl * dl * (na * nb / n);
  ma = ma + dl * (nb / n);
  na = n;
}

// mom[seg][4][C * D]: mean / M2 of the segment's rows inside the first half [0, h), mean / M2 of those inside the last half [S - h, S)
template <typename T>
__global__ void __launch_bounds__(DIAG_THREADS) diag_moments_kernel(const T* __restrict__ x, int64_t ss, int64_t sc, int64_t S, int64_t C, int64_t D,
                                                                    double* __restrict__ mom) {
  const int64_t j = blockIdx.x * (int64_t)DIAG_THREADS + threadIdx.x, CD = C * D;
  if (j >= CD) return;
  const int64_t c = j / D, d = j - c * D, h = S / 2;
  const int64_t r0 = (int64_t)blockIdx.y * DIAG_SEGMENT_ROWS, r1 = r0 + DIAG_SEGMENT_ROWS < S ? r0 + DIAG_SEGMENT_ROWS : S;
  const T* xs = x + c * sc + d;
  double* out = mom + (int64_t)blockIdx.y * 4 * CD + j;
  double m, q;
  diag_rows(xs, ss, r0, r1 < h ? r1 : h, m, q);
  out[0] = m; out[CD] = q;
  diag_rows(xs, ss, r0 > S - h ? r0 : S - h, r1, m, q);
  out[2 * CD] = m; out[3 * CD] = q;
}

struct DiagSeries { double mean, m2, ma, qa, mb, qb; };   // whole chain, first half, last half

template <typename T>
__device__ __forceinline__ DiagSeries diag_series(const T* __restrict__ x, int64_t ss, int64_t sc, int64_t S, int64_t C, int64_t D, int64_t nseg,
                                                  const double* __restrict__ mom, int64_t c, int64_t d) {
  const int64_t CD = C * D, j = c * D + d, h = S / 2;
  double na = 0.0, ma = 0.0, qa = 0.0, nb = 0.0, mb = 0.0, qb = 0.0;
  for (int64_t g = 0; g < nseg; ++g) {
    const int64_t r0 = g * DIAG_SEGMENT_ROWS, r1 = r0 + DIAG_SEGMENT_ROWS < S ? r0 + DIAG_SEGMENT_ROWS : S;
    const int64_t a1 = r1 < h ? r1 : h, b0 = r0 > S - h ? r0 : S - h;
    const double* p = mom + g * 4 * CD + j;
    if (a1 > r0) diag_chan(na, ma, qa, (double)(a1 - r0), p[0], p[CD]);
    if (r1 > b0) diag_chan(nb, mb, qb, (double)(r1 - b0), p[2 * CD], p[3 * CD]);
  }
  DiagSeries r;
  r.ma = ma; r.qa = qa; r.mb = mb; r.qb = qb;
  double n = na, m = ma, q = qa;
  if (S & 1) diag_chan(n, m, q, 1.0, (double)x[h * ss + c * sc + d], 0.0);     // the middle row of an odd S belongs to neither half
  diag_chan(n, m, q, nb, mb, qb);
  r.mean = m; r.m2 = q;
  return r;
}

// one block per coordinate: chain statistics -> mean, sd, R-hat, and the walk's start (tau, t, done) = (-1, 0, 0)
template <typename T>
__global__ void __launch_bounds__(DIAG_THREADS) diag_combine_kernel(const T* __restrict__ x, int64_t ss, int64_t sc, int64_t S, int64_t C, int64_t D, int64_t nseg,
                                                                    const double* __restrict__ mom, double* __restrict__ series_mean,
                                                                    double* __restrict__ mean_var, double* __restrict__ var_plus, double* __restrict__ tau,
                                                                    int32_t* __restrict__ t_state, int32_t* __restrict__ done,
                                                                    double* __restrict__ mean_out, double* __restrict__ sd_out, double* __restrict__ rhat_out) {
  __shared__ double red[6][DIAG_THREADS];
  const int64_t d = blockIdx.x;
  const int tid = threadIdx.x;
  const DiagSeries z = diag_series(x, ss, sc, S, C, D, nseg, mom, 0, d);       // chain 0: the shift of the sums over chains
  double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t c = tid; c < C; c += DIAG_THREADS) {
    const DiagSeries r = diag_series(x, ss, sc, S, C, D, nseg, mom, c, d);
    series_mean[c * D + d] = r.mean;
    const double dm = r.mean - z.mean, da = r.ma - z.ma, db = r.mb - z.ma;
    a[0] += dm; a[1] += dm * dm; a[2] += r.m2;
    a[3] += da + db; a[4] += da * da + db * db; a[5] += r.qa + r.qb;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) red[i][tid] = a[i];
  __syncthreads();
  for (int o = DIAG_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int i = 0; i < 6; ++i) red[i][tid] += red[i][tid + o];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const double n = (double)S, nc = (double)C, h = (double)(S / 2);
  const double mv = red[2][0] / (n - 1.0) / nc;
  double vp = mv * (n - 1.0) / n;
  if (C > 1) {
    double between = (red[1][0] - red[0][0] * red[0][0] / nc) / (nc - 1.0);
    vp += between < 0.0 ? 0.0 : between;
  }
  mean_var[d] = mv;
  var_plus[d] = vp;
  tau[d] = -1.0;
  t_state[d] = 0;
  done[d] = 0;
  mean_out[d] = z.mean + red[0][0] / nc;
  sd_out[d] = sqrt(vp);
  // split R-hat over the 2 C half chains (ess.py: rhat_split)
  double rh = __builtin_nan("");
  if (h >= 2.0) {
    const double n2 = 2.0 * nc;
    const double w = red[5][0] / (h - 1.0) / n2;
    double vb = (red[4][0] - red[3][0] * red[3][0] / n2) / (n2 - 1.0);
    if (vb < 0.0) vb = 0.0;
    const double b = h * vb;
    if (w <= 0.0) rh = b > 0.0 ? __builtin_inf() : __builtin_nan("");
    else rh = sqrt(((h - 1.0) / h * w + b / h) / w);
  }
  rhat_out[d] = rh;
}

template <int B>
__device__ __forceinline__ void diag_lag_step(double a, double l, double (&w)[B], double (&acc)[B]) {
#pragma unroll
  for (int i = B - 1; i > 0; --i) w[i] = w[i - 1];
  w[0] = l;
#pragma unroll
  for (int k = 0; k < B; ++k) acc[k] = fma(a, w[k], acc[k]);
}

// part[lag][seg * G + cg][d] = sum over the chains of group cg and the lead rows u of segment seg of xc[u] xc[u - lag],
// lag = t0 + B blockIdx.z + k.  The window w[i] = xc[u - lag0 - i] moves one row per step.
template <typename T, int B>
__global__ void __launch_bounds__(DIAG_THREADS, 4) diag_lags_kernel(const T* __restrict__ x, int64_t ss, int64_t sc, int64_t S, int64_t C, int64_t D, int64_t G,
                                                                    const double* __restrict__ series_mean, int64_t t0, double* __restrict__ part) {
  const int64_t p = blockIdx.x * (int64_t)DIAG_THREADS + threadIdx.x;
  if (p >= G * D) return;
  const int64_t cg = p / D, d = p - cg * D;
  const int64_t lag0 = t0 + (int64_t)blockIdx.z * B;
  const int64_t r0 = (int64_t)blockIdx.y * DIAG_SEGMENT_ROWS, r1 = r0 + DIAG_SEGMENT_ROWS < S ? r0 + DIAG_SEGMENT_ROWS : S;
  const int64_t u0 = r0 > lag0 ? r0 : lag0;                   // a lead row below lag0 has no partner
  constexpr int U = 4;                                          // rows per batch of loads (8 in flight: 16 spill in the f32 instance)
  double acc[B], w[B];
#pragma unroll
  for (int k = 0; k < B; ++k) acc[k] = 0.0;
  if (u0 < r1) {
    for (int64_t c = cg; c < C; c += G) {
      const T* xs = x + c * sc + d;
      const double mu = series_mean[c * D + d];
#pragma unroll
      for (int i = 0; i < B - 1; ++i) {                        // w[i] = xc[u0 - lag0 - 1 - i]: shifted into place by the first step
        const int64_t s = u0 - lag0 - 1 - i;
        w[i] = s >= 0 ? (double)xs[s * ss] - mu : 0.0;
      }
      w[B - 1] = 0.0;
      const T* xl = xs - lag0 * ss;                            // the lagged stream (the lead's own rows, from cache, when lag0 == 0)
      int64_t u = u0;
      for (; u + U <= r1; u += U) {                            // U rows of both streams in flight, then their U B products
        T la[U], ll[U];
#pragma unroll
        for (int i = 0; i < U; ++i) { la[i] = xs[(u + i) * ss]; ll[i] = xl[(u + i) * ss]; }
#pragma unroll
        for (int i = 0; i < U; ++i) diag_lag_step<B>((double)la[i] - mu, (double)ll[i] - mu, w, acc);
      }
      for (; u < r1; ++u) diag_lag_step<B>((double)xs[u * ss] - mu, (double)xl[u * ss] - mu, w, acc);
    }
  }
  const int64_t P = (int64_t)gridDim.y * G;
  double* out = part + ((int64_t)blockIdx.z * B * P + (int64_t)blockIdx.y * G) * D + p;
#pragma unroll
  for (int k = 0; k < B; ++k) out[k * P * D] = acc[k];
}

// acov[l][d] = sum over the P partial rows, in order: 16 coordinates x 16 row slices per block, the slices merged through LDS
__global__ void __launch_bounds__(DIAG_THREADS) diag_lag_reduce_kernel(const double* __restrict__ part, int64_t P, int64_t D, double* __restrict__ acov) {
  __shared__ double red[16][17];
  const int dx = threadIdx.x & 15, ry = threadIdx.x >> 4;
  const int64_t d = blockIdx.x * (int64_t)16 + dx, l = blockIdx.y;
  double a = 0.0;
  if (d < D) {
    const double* p = part + l * P * D + d;
    for (int64_t r = ry; r < P; r += 16) a += p[r * D];
  }
  red[ry][dx] = a;
  __syncthreads();
  if (ry == 0 && d < D) {
    double s = red[0][dx];
#pragma unroll
    for (int i = 1; i < 16; ++i) s += red[i][dx];
    acov[l * D + d] = s;
  }
}

// The Geyer walk of every coordinate over the lags [t0, t0 + n_lags) of acov (raw sums: divided by S C here), stopped in front of
// lag_limit (the caller's max_lag) without being marked done.
__global__ void __launch_bounds__(DIAG_THREADS) diag_finish_kernel(const double* __restrict__ acov, int64_t S, int64_t C, int64_t D, int64_t t0, int64_t n_lags, int64_t lag_limit,
                                                                   const double* __restrict__ mean_var, const double* __restrict__ var_plus, double* __restrict__ tau,
                                                                   int32_t* __restrict__ t_state, int32_t* __restrict__ done, double* __restrict__ tau_out,
                                                                   double* __restrict__ ess_out, int32_t* __restrict__ lags_out, int32_t* __restrict__ done_out,
                                                                   int32_t* __restrict__ not_done) {
  const int64_t d = blockIdx.x * (int64_t)DIAG_THREADS + threadIdx.x;
  int open = 0;
  if (d < D) {
    const double mv = mean_var[d], vp = var_plus[d], sc = (double)S * (double)C;
    double ta = tau[d];
    int64_t t = t_state[d];
    int dn = done[d];
    if (!dn && !(vp > 0.0 && vp < __builtin_inf())) {         // zero, infinite or NaN spread: no autocorrelation to walk
      dn = 1;
      ta = __builtin_nan("");
    } else if (!dn) {
      const int64_t end = t0 + n_lags < lag_limit ? t0 + n_lags : lag_limit;
      const int64_t lim = end < S ? end : S;                    // the lags this call may read: t0 <= lag < lim
      bool open_walk = true;
      while (open_walk) {
        if (t + 1 >= S) { dn = 1; break; }
        if (t + 1 >= end || t < t0) break;
        double r[16];                                           // eight pairs in flight, then walked in order
#pragma unroll
        for (int i = 0; i < 16; ++i) r[i] = t + i < lim ? acov[(t + i - t0) * D + d] : 0.0;
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
          if (open_walk && t + 1 < lim) {
            const double r0 = t == 0 ? 1.0 : 1.0 - (mv - r[i] / sc) / vp;
            const double r1 = 1.0 - (mv - r[i + 1] / sc) / vp;
            const double pair = r0 + r1;
            if (pair < 0.0) { dn = 1; open_walk = false; }
            else if (!(pair >= 0.0)) { dn = 1; ta = __builtin_nan(""); open_walk = false; }
            else { ta += 2.0 * pair; t += 2; }
          }
        }
      }
    }
    tau[d] = ta;
    t_state[d] = (int32_t)t;
    done[d] = dn;
    const double fl = 1.0 / log10(sc + 10.0);
    const double tf = ta != ta ? ta : (ta > fl ? ta : fl);
    tau_out[d] = tf;
    ess_out[d] = sc / tf;
    lags_out[d] = (int32_t)t;
    done_out[d] = dn;
    open = !dn;
  }
  const int n = __syncthreads_count(open);
  if (threadIdx.x == 0 && n) atomicAdd(not_done, n);
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------
static int diag_check(const char* who, const void* x, int64_t ss, int64_t sc, int64_t S, int64_t C, int64_t D) {
  HTA_REQUIRE(x && S >= 4 && C >= 1 && D >= 1 && S < (1ll << 31) && D < (1ll << 31) && C < (1ll << 31), "%s: bad shape (S=%lld C=%lld D=%lld)", who, (long long)S,
              (long long)C, (long long)D);
  HTA_REQUIRE(sc >= D && ss >= (C - 1) * sc + D, "%s: bad strides (stride_s=%lld stride_c=%lld): rows and chains must not overlap", who, (long long)ss,
              (long long)sc);
  HTA_REQUIRE((S + DIAG_SEGMENT_ROWS - 1) / DIAG_SEGMENT_ROWS <= 65535, "%s: S=%lld is beyond 65535 segments of %d rows", who, (long long)S, DIAG_SEGMENT_ROWS);
  return HTA_OK;
}
static int diag_check_ws(const char* who, const void* ws, int64_t bytes, int64_t need_words) {
  HTA_REQUIRE(ws && ((uintptr_t)ws & 7) == 0 && bytes >= 8 * need_words, "%s: workspace of %lld bytes (8-byte aligned) needed, %lld given", who,
              (long long)(8 * need_words), (long long)bytes);
  return HTA_OK;
}

template <typename T>
static int diag_moments(const T* x, int64_t ss, int64_t sc, int64_t S, int64_t C, int64_t D, double* mean, double* sd, double* rhat, void* workspace,
                        int64_t workspace_bytes, void* stream) {
  if (int rc = diag_check("hta_diag_moments", x, ss, sc, S, C, D)) return rc;
  HTA_REQUIRE(mean && sd && rhat, "hta_diag_moments: an output pointer is NULL");
  const DiagLayout L = diag_layout(S, C, D);
  if (int rc = diag_check_ws("hta_diag_moments", workspace, workspace_bytes, diag_words(L, D, 0))) return rc;
  double* w = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((C * D + DIAG_THREADS - 1) / DIAG_THREADS), (unsigned)L.nseg);
  diag_moments_kernel<T><<<grid, DIAG_THREADS, 0, st>>>(x, ss, sc, S, C, D, w + L.mom);
  HTA_CHECK_LAUNCH("diag_moments_kernel");
  diag_combine_kernel<T><<<(unsigned)D, DIAG_THREADS, 0, st>>>(x, ss, sc, S, C, D, L.nseg, w + L.mom, w + L.series_mean, w + L.mean_var, w + L.var_plus, w + L.tau,
                                                              (int32_t*)(w + L.t), (int32_t*)(w + L.done), mean, sd, rhat);
  HTA_CHECK_LAUNCH("diag_combine_kernel");
  return HTA_OK;
}

template <typename T>
static int diag_lags(const T* x, int64_t ss, int64_t sc, int64_t S, int64_t C, int64_t D, int64_t t0, int n_lags, void* workspace, int64_t workspace_bytes,
                     void* stream) {
  if (int rc = diag_check("hta_diag_lags", x, ss, sc, S, C, D)) return rc;
  HTA_REQUIRE(t0 >= 0 && t0 < S && t0 % DIAG_LAG_BLOCK == 0 && n_lags > 0 && n_lags % DIAG_LAG_BLOCK == 0 && n_lags <= DIAG_LAG_BLOCK * DIAG_MAX_LAG_BLOCKS,
              "hta_diag_lags: bad lag range (t0=%lld n_lags=%d): whole blocks of %d lags, at most %d per call, t0 < S", (long long)t0, n_lags, DIAG_LAG_BLOCK,
              DIAG_MAX_LAG_BLOCKS);
  const DiagLayout L = diag_layout(S, C, D);
  if (int rc = diag_check_ws("hta_diag_lags", workspace, workspace_bytes, diag_words(L, D, n_lags))) return rc;
  double* w = (double*)workspace;
  double* acov = w + L.acov;
  double* part = acov + (int64_t)n_lags * D;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((L.G * D + DIAG_THREADS - 1) / DIAG_THREADS), (unsigned)L.nseg, (unsigned)(n_lags / DIAG_LAG_BLOCK));
  note_route("diag_lags_kernel<%s,%d>", sizeof(T) == 4 ? "float" : "double", DIAG_LAG_BLOCK);
  diag_lags_kernel<T, DIAG_LAG_BLOCK><<<grid, DIAG_THREADS, 0, st>>>(x, ss, sc, S, C, D, L.G, w + L.series_mean, t0, part);
  HTA_CHECK_LAUNCH("diag_lags_kernel");
  diag_lag_reduce_kernel<<<dim3((unsigned)((D + 15) / 16), (unsigned)n_lags), DIAG_THREADS, 0, st>>>(part, L.P, D, acov);
  HTA_CHECK_LAUNCH("diag_lag_reduce_kernel");
  return HTA_OK;
}

}  // namespace hta

extern "C" {

int hta_diag_lag_block(void) { return hta::DIAG_LAG_BLOCK; }
int hta_diag_segment_rows(void) { return hta::DIAG_SEGMENT_ROWS; }

int64_t hta_diag_workspace_bytes(int64_t S, int64_t C, int64_t D, int n_lags) {
  if (S < 1 || C < 1 || D < 1 || n_lags < 0) return -1;
  return 8 * hta::diag_words(hta::diag_layout(S, C, D), D, n_lags);
}

int hta_diag_moments_f32(const float* x, int64_t stride_s, int64_t stride_c, int64_t S, int64_t C, int64_t D, double* mean, double* sd, double* rhat,
                         void* workspace, int64_t workspace_bytes, void* stream) {
  return hta::diag_moments<float>(x, stride_s, stride_c, S, C, D, mean, sd, rhat, workspace, workspace_bytes, stream);
}
int hta_diag_moments_f64(const double* x, int64_t stride_s, int64_t stride_c, int64_t S, int64_t C, int64_t D, double* mean, double* sd, double* rhat,
                         void* workspace, int64_t workspace_bytes, void* stream) {
  return hta::diag_moments<double>(x, stride_s, stride_c, S, C, D, mean, sd, rhat, workspace, workspace_bytes, stream);
}
int hta_diag_lags_f32(const float* x, int64_t stride_s, int64_t stride_c, int64_t S, int64_t C, int64_t D, int64_t t0, int n_lags, void* workspace,
                      int64_t workspace_bytes, void* stream) {
  return hta::diag_lags<float>(x, stride_s, stride_c, S, C, D, t0, n_lags, workspace, workspace_bytes, stream);
}
int hta_diag_lags_f64(const double* x, int64_t stride_s, int64_t stride_c, int64_t S, int64_t C, int64_t D, int64_t t0, int n_lags, void* workspace,
                      int64_t workspace_bytes, void* stream) {
  return hta::diag_lags<double>(x, stride_s, stride_c, S, C, D, t0, n_lags, workspace, workspace_bytes, stream);
}

int hta_diag_finish(int64_t S, int64_t C, int64_t D, int64_t t0, int n_lags, int64_t lag_limit, double* tau, double* ess, int32_t* lags_used, int32_t* done,
                    int32_t* not_done, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace hta;
  HTA_REQUIRE(S >= 4 && C >= 1 && D >= 1 && S < (1ll << 31) && D < (1ll << 31) && C < (1ll << 31), "hta_diag_finish: bad shape (S=%lld C=%lld D=%lld)", (long long)S,
              (long long)C, (long long)D);
  HTA_REQUIRE(t0 >= 0 && t0 % DIAG_LAG_BLOCK == 0 && n_lags > 0 && n_lags % DIAG_LAG_BLOCK == 0 && n_lags <= DIAG_LAG_BLOCK * DIAG_MAX_LAG_BLOCKS && lag_limit >= 1,
              "hta_diag_finish: bad lag range (t0=%lld n_lags=%d lag_limit=%lld)", (long long)t0, n_lags, (long long)lag_limit);
  HTA_REQUIRE(tau && ess && lags_used && done && not_done, "hta_diag_finish: an output pointer is NULL");
  const DiagLayout L = diag_layout(S, C, D);
  if (int rc = diag_check_ws("hta_diag_finish", workspace, workspace_bytes, diag_words(L, D, n_lags))) return rc;
  double* w = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(not_done, 0, sizeof(int32_t), st) != hipSuccess) { set_error("hta_diag_finish: hipMemsetAsync failed"); return HTA_ERR_LAUNCH; }
  diag_finish_kernel<<<(unsigned)((D + DIAG_THREADS - 1) / DIAG_THREADS), DIAG_THREADS, 0, st>>>(w + L.acov, S, C, D, t0, n_lags, lag_limit, w + L.mean_var, w + L.var_plus,
                                                                                               w + L.tau, (int32_t*)(w + L.t), (int32_t*)(w + L.done), tau, ess,
                                                                                               lags_used, done, not_done);
  HTA_CHECK_LAUNCH("diag_finish_kernel");
  return HTA_OK;
}

}  // extern "C"
