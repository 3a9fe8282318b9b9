// Rank-normalisation of batched chains on the device (Vehtari et al. 2021): for every coordinate d of samples x[S, C, D] the
// average ranks of its N = S C draws, z = Phi^-1((r - 3/8) / (N + 1/4)), the indicators of the 5 % and 95 % order statistics, the
// quantiles, and the same z for the folded draws |x - med|.  The derived series go through the stages of csrc/diagnostics.hip.
//
//   gather     diag_rank_gather_kernel<T, K, FOLD>: column d of x (unit stride in d, element strides for s and c: views are read in
//              place) -> keys[d][n], n = s C + c, and the payload n.  float -> order-preserving uint32, double and the fold's fp64
//              |x - centre| -> uint64; -0.0 counts as +0.0.  Non-finite values are counted per coordinate (an integer atomic).
//   sort       LSD radix sort, 8-bit digits, one segment per coordinate, a tile of DIAG_RANK_TILE keys per block and pass.  A pass is
//              three launches: diag_rank_hist_kernel (digit counts per tile, LDS integer atomics), diag_rank_scan_kernel (a block
//              per coordinate: exclusive scan over (digit, tile) in place) and diag_rank_scatter_kernel (stable: the keys of a tile
//              in rounds of one per thread, equal digits ranked inside a wave by __ballot, waves and rounds in order through LDS
//              counters).  The coordinate is part of the flat grid index.  Passes are separated by kernel boundaries: no
//              workgroup ever waits for another.
//   transform  diag_rank_transform_kernel<K, FIRST>: a thread per sorted position j; the tie run [lo, hi) of its key by a galloping
//              search in both directions (runs may cross tiles: the search reads the sorted keys, it needs no neighbour block),
//              r = (lo + hi + 1) / 2, z scattered by the payload into z[S, C, D].  FIRST also writes I05 / I95 (float: exact) and
//              thread 0 of a coordinate its quantiles (numpy's linear interpolation) and the fold's centre 0.5 (x_((N-1)/2) + x_(N/2)).
//   Phi^-1     Wichura's algorithm AS 241, routine PPND16 (Appl. Statist. 37, 1988), relative error about 1e-16, in fp64; without its
//              far-tail range p < exp(-25) = 1.4e-11, which (r - 3/8) / (N + 1/4) >= 2.9e-10 never enters.
//
// Integer atomics only, and only on counts whose order cannot change a result; the sort is stable and tie-averaged ranks do not
// depend on the order inside a run: equal inputs give equal bits whatever D, the strides or the chunking.  Nothing here allocates
// or synchronises.
#include "common.hpp"

namespace hta {

constexpr int DIAG_RANK_THREADS = 256;
constexpr int DIAG_RANK_ITEMS = 8;                                        // keys per thread, tile and pass
constexpr int DIAG_RANK_TILE = DIAG_RANK_THREADS * DIAG_RANK_ITEMS;       // T: keys per block and pass
constexpr int DIAG_RANK_WAVES = DIAG_RANK_THREADS / 64;
constexpr int DIAG_RANK_SCAN_THREADS = 1024;                              // 256 digits x 4 slices of the tiles

// AS 241 PPND16: the normal deviate of lower tail area p, its central and intermediate ranges: exp(-25) <= p <= 1 - exp(-25), NaN outside
__host__ __device__ inline double diag_ndtri(double p) {
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    return q * (((((((r * 2509.0809287301226727 + 33430.575583588128105) * r + 67265.770927008700853) * r + 45921.953931549871457) * r +
                   13731.693765509461125) * r + 1971.5909503065514427) * r + 133.14166789178437745) * r + 3.387132872796366608) /
           (((((((r * 5226.495278852545925 + 28729.085735721942674) * r + 39307.89580009271061) * r + 21213.794301586595867) * r +
               5394.1960214247511077) * r + 687.1870074920579083) * r + 42.313330701600911252) * r + 1.0);
  }
  double r = sqrt(-log(q < 0.0 ? p : 1.0 - p));
  if (r > 5.0) return __builtin_nan("");                        // min(p, 1 - p) < exp(-25): not reached, N < 2^31 keeps it above 2.9e-10
  r -= 1.6;
  const double v = (((((((r * 7.7454501427834140764e-4 + 0.0227238449892691845833) * r + 0.24178072517745061177) * r + 1.27045825245236838258) * r +
                       3.64784832476320460504) * r + 5.7694972214606914055) * r + 4.6303378461565452959) * r + 1.42343711074968357734) /
                   (((((((r * 1.05075007164441684324e-9 + 5.475938084995344946e-4) * r + 0.0151986665636164571966) * r + 0.14810397642748007459) * r +
                       0.68976733498510000455) * r + 1.6763848301838038494) * r + 2.05319162663775882187) * r + 1.0);
  return q < 0.0 ? -v : v;
}

// order-preserving keys: sign bit flipped for positive values, all bits for negative ones; both zeros give the key of +0.0
__device__ __forceinline__ uint32_t diag_rank_encode(float v) {
  uint32_t b = __float_as_uint(v);
  if ((b << 1) == 0u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ uint64_t diag_rank_encode(double v) {
  uint64_t b = (uint64_t)__double_as_longlong(v);
  if ((b << 1) == 0ull) b = 0ull;
  return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double diag_rank_decode(uint32_t k) {
  return (double)__uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ double diag_rank_decode(uint64_t k) {
  return __longlong_as_double((long long)((k & 0x8000000000000000ull) ? (k ^ 0x8000000000000000ull) : ~k));
}

// the flat grid: block b works on tile b % nblk of coordinate b / nblk
struct DiagRankTile { int64_t d; uint32_t first; };
__device__ __forceinline__ DiagRankTile diag_rank_tile(uint32_t nblk) {
  DiagRankTile t;
  t.d = blockIdx.x / nblk;
  t.first = (blockIdx.x - (uint32_t)t.d * nblk) * (uint32_t)DIAG_RANK_TILE;
  return t;
}

template <typename T, typename K, bool FOLD>
__global__ void __launch_bounds__(DIAG_RANK_THREADS) diag_rank_gather_kernel(const T* __restrict__ x, int64_t ss, int64_t sc, uint32_t N, uint32_t C, uint32_t nblk,
                                                                             const double* __restrict__ centre, K* __restrict__ keys, uint32_t* __restrict__ idx,
                                                                             int32_t* __restrict__ bad) {
  const DiagRankTile t = diag_rank_tile(nblk);
  const T* xd = x + t.d;
  K* kd = keys + t.d * N;
  uint32_t* id = idx + t.d * N;
  double mid = 0.0;
  if (FOLD) mid = centre[t.d];
  int nonfinite = 0;
#pragma unroll
  for (int i = 0; i < DIAG_RANK_ITEMS; ++i) {
    const uint32_t n = t.first + (uint32_t)i * DIAG_RANK_THREADS + threadIdx.x;
    if (n < N) {
      const uint32_t s = n / C, c = n - s * C;
      const T v = xd[(int64_t)s * ss + (int64_t)c * sc];
      if (FOLD) {
        const double f = fabs((double)v - mid);
        nonfinite += !(f < __builtin_inf());
        kd[n] = (K)diag_rank_encode(f);
      } else {
        nonfinite += !(fabs((double)v) < __builtin_inf());
        kd[n] = (K)diag_rank_encode(v);
      }
      id[n] = n;
    }
  }
  if (nonfinite) atomicAdd(bad + t.d, nonfinite);
}

// hist[d][tile][digit]: how many keys of the tile have the digit
template <typename K>
__global__ void __launch_bounds__(DIAG_RANK_THREADS) diag_rank_hist_kernel(const K* __restrict__ keys, uint32_t N, uint32_t nblk, int shift, uint32_t* __restrict__ hist) {
  __shared__ uint32_t cnt[256];
  const DiagRankTile t = diag_rank_tile(nblk);
  const K* kd = keys + t.d * N;
  cnt[threadIdx.x] = 0u;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < DIAG_RANK_ITEMS; ++i) {
    const uint32_t n = t.first + (uint32_t)i * DIAG_RANK_THREADS + threadIdx.x;
    if (n < N) atomicAdd(&cnt[(uint32_t)(kd[n] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(int64_t)blockIdx.x * 256 + threadIdx.x] = cnt[threadIdx.x];
}

// a block per coordinate: hist[d][tile][digit] <- the number of keys with a smaller digit, or with this digit in an earlier tile.
// Thread (slice, digit) sums the tiles of its quarter; the 256 digit totals are scanned in LDS; the second sweep writes the offsets.
__global__ void __launch_bounds__(DIAG_RANK_SCAN_THREADS) diag_rank_scan_kernel(uint32_t* __restrict__ hist, uint32_t nblk) {
  __shared__ uint32_t tot[4][256];
  __shared__ uint32_t scan[256];
  const uint32_t digit = threadIdx.x & 255u, slice = threadIdx.x >> 8;
  uint32_t* h = hist + (int64_t)blockIdx.x * nblk * 256 + digit;
  const uint32_t per = (nblk + 3u) / 4u;
  const uint32_t b0 = slice * per < nblk ? slice * per : nblk, b1 = b0 + per < nblk ? b0 + per : nblk;
  uint32_t sum = 0u;
#pragma unroll 8
  for (uint32_t b = b0; b < b1; ++b) sum += h[(int64_t)b * 256];
  tot[slice][digit] = sum;
  __syncthreads();
  const uint32_t all = tot[0][digit] + tot[1][digit] + tot[2][digit] + tot[3][digit];
  if (slice == 0u) scan[digit] = all;
  __syncthreads();
  for (uint32_t o = 1u; o < 256u; o <<= 1) {
    uint32_t v = 0u;
    if (slice == 0u && digit >= o) v = scan[digit - o];
    __syncthreads();
    if (slice == 0u) scan[digit] += v;
    __syncthreads();
  }
  uint32_t run = scan[digit] - all;                             // (inclusive -> exclusive)
  for (uint32_t s = 0u; s < slice; ++s) run += tot[s][digit];
  for (uint32_t b = b0; b < b1; b += 8u) {                       // eight counts in flight, then their offsets
    uint32_t v[8];
#pragma unroll
    for (uint32_t i = 0u; i < 8u; ++i) v[i] = b + i < b1 ? h[(int64_t)(b + i) * 256] : 0u;
#pragma unroll
    for (uint32_t i = 0u; i < 8u; ++i) {
      if (b + i < b1) h[(int64_t)(b + i) * 256] = run;
      run += v[i];
    }
  }
}

// stable scatter of a tile: round i takes the keys first + 256 i + tid.  Within a wave equal digits are ranked by lane (eight ballots
// give every lane the mask of its peers), the waves of a round and the rounds of a tile follow each other through wcnt / base.
template <typename K>
__global__ void __launch_bounds__(DIAG_RANK_THREADS) diag_rank_scatter_kernel(const K* __restrict__ kin, const uint32_t* __restrict__ iin, K* __restrict__ kout,
                                                                              uint32_t* __restrict__ iout, uint32_t N, uint32_t nblk, int shift,
                                                                              const uint32_t* __restrict__ hist) {
  __shared__ uint32_t base[256];
  __shared__ uint32_t wcnt[DIAG_RANK_WAVES][256];
  const DiagRankTile t = diag_rank_tile(nblk);
  const K* ki = kin + t.d * N;
  const uint32_t* ii = iin + t.d * N;
  K* ko = kout + t.d * N;
  uint32_t* io = iout + t.d * N;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  base[tid] = hist[(int64_t)blockIdx.x * 256 + tid];
#pragma unroll
  for (int k = 0; k < DIAG_RANK_WAVES; ++k) wcnt[k][tid] = 0u;
  __syncthreads();
  for (int i = 0; i < DIAG_RANK_ITEMS; ++i) {
    const uint32_t n0 = t.first + (uint32_t)i * DIAG_RANK_THREADS;
    if (n0 >= N) break;                                         // (the same for the whole block)
    const uint32_t n = n0 + tid;
    const bool active = n < N;
    K key = 0;
    uint32_t payload = 0u;
    if (active) { key = ki[n]; payload = ii[n]; }
    const uint32_t digit = (uint32_t)(key >> shift) & 255u;
    unsigned long long peers = __ballot(active);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (digit >> b) & 1u;
      const unsigned long long m = __ballot(active && bit);
      peers &= bit ? m : ~m;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
    if (active && rank == 0u) wcnt[w][digit] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (active) {
      uint32_t pos = base[digit] + rank;
      for (uint32_t k = 0u; k < w; ++k) pos += wcnt[k][digit];
      if (pos < N) {                                            // (always: the offsets count exactly these keys)
        ko[pos] = key;
        io[pos] = payload;
      }
    }
    __syncthreads();
    uint32_t add = 0u;
#pragma unroll
    for (int k = 0; k < DIAG_RANK_WAVES; ++k) { add += wcnt[k][tid]; wcnt[k][tid] = 0u; }
    base[tid] += add;
    __syncthreads();
  }
}

// numpy.quantile(method="linear") of the sorted keys: the virtual index n q + (1 - q) - 1 as numpy forms it, and its _lerp
template <typename K>
__device__ __forceinline__ double diag_rank_quantile(const K* __restrict__ kd, uint32_t N, double q) {
  const double h = (double)N * q + (1.0 + q * -1.0) - 1.0;
  double fl = floor(h);
  if (fl < 0.0) fl = 0.0;
  uint32_t lo = (uint32_t)fl;
  if (lo > N - 1u) lo = N - 1u;
  const uint32_t hi = lo + 1u < N ? lo + 1u : N - 1u;
  const double g = h - fl, a = diag_rank_decode(kd[lo]), b = diag_rank_decode(kd[hi]), df = b - a;
  return g >= 0.5 ? b - df * (1.0 - g) : a + df * g;
}

template <typename K, bool FIRST>
__global__ void __launch_bounds__(DIAG_RANK_THREADS) diag_rank_transform_kernel(const K* __restrict__ keys, const uint32_t* __restrict__ idx, uint32_t N, uint32_t nblk, int64_t D,
                                                                                const int32_t* __restrict__ bad, double* __restrict__ z_out, float* __restrict__ i05_out,
                                                                                float* __restrict__ i95_out, double* __restrict__ q05, double* __restrict__ median,
                                                                                double* __restrict__ q95, double* __restrict__ centre) {
  const DiagRankTile t = diag_rank_tile(nblk);
  const K* kd = keys + t.d * N;
  const uint32_t* id = idx + t.d * N;
  const bool degenerate = bad[t.d] != 0;
  const double nan = __builtin_nan("");
  K k05 = 0, k95 = 0;
  if (FIRST) {
    k05 = kd[(N - 1u) / 20u];
    k95 = kd[(uint32_t)((uint64_t)19u * (N - 1u) / 20u)];
    if (t.first == 0u && threadIdx.x == 0u) {
      q05[t.d] = degenerate ? nan : diag_rank_quantile(kd, N, 0.05);
      median[t.d] = degenerate ? nan : diag_rank_quantile(kd, N, 0.5);
      q95[t.d] = degenerate ? nan : diag_rank_quantile(kd, N, 0.95);
      centre[t.d] = degenerate ? nan : 0.5 * (diag_rank_decode(kd[(N - 1u) / 2u]) + diag_rank_decode(kd[N / 2u]));
    }
  }
  const double denom = (double)N + 0.25;
  for (int i = 0; i < DIAG_RANK_ITEMS; ++i) {
    const uint32_t j = t.first + (uint32_t)i * DIAG_RANK_THREADS + threadIdx.x;
    if (j >= N) break;
    const K key = kd[j];
    // [lo, hi): the positions that hold this key.  a always holds it, l never does (or lies outside the segment)
    int64_t a = j, l = -1, st = 1;
    if (j > 0u && kd[j - 1u] == key) {
      for (;;) {
        const int64_t p = a - st;
        if (p < 0) { l = -1; break; }
        if (kd[p] == key) { a = p; st <<= 1; } else { l = p; break; }
      }
      while (a - l > 1) {
        const int64_t m = (a + l) >> 1;
        if (kd[m] == key) a = m; else l = m;
      }
    }
    const int64_t lo = a;
    a = j; st = 1; l = N;
    if (j + 1u < N && kd[j + 1u] == key) {
      for (;;) {
        const int64_t p = a + st;
        if (p >= (int64_t)N) { l = N; break; }
        if (kd[p] == key) { a = p; st <<= 1; } else { l = p; break; }
      }
      while (l - a > 1) {
        const int64_t m = (a + l) >> 1;
        if (kd[m] == key) a = m; else l = m;
      }
    }
    const int64_t hi = a + 1;
    const double r = 0.5 * (double)(lo + hi + 1);               // the mean of the 1-based ranks lo + 1 .. hi
    const uint32_t n = id[j];
    if (n >= N) continue;                                       // (never: the payloads are a permutation of 0 .. N - 1)
    const int64_t o = (int64_t)n * D + t.d;
    z_out[o] =degenerate ? nan : diag_ndtri((r - 0.375) / denom);
    if (FIRST) {
      i05_out[o] = degenerate ? __builtin_nanf("") : (key <= k05 ? 1.0f : 0.0f);
      i95_out[o] = degenerate ? __builtin_nanf("") : (key <= k95 ? 1.0f : 0.0f);
    }
  }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------
struct DiagRankLayout { int64_t nblk, keys_a, keys_b, idx_a, idx_b, hist, total; };      // byte offsets (8-byte aligned)

static DiagRankLayout diag_rank_layout(int64_t N, int64_t D, int64_t key_bytes) {
  DiagRankLayout L;
  const int64_t kb = (N * D * key_bytes + 7) / 8 * 8, ib = (N * D * 4 + 7) / 8 * 8;
  L.nblk = (N + DIAG_RANK_TILE - 1) / DIAG_RANK_TILE;
  L.keys_a = 0;
  L.keys_b = L.keys_a + kb;
  L.idx_a = L.keys_b + kb;
  L.idx_b = L.idx_a + ib;
  L.hist = L.idx_b + ib;
  L.total = L.hist + D * L.nblk * 256 * 4;
  return L;
}

static int diag_rank_check(const char* who, const void* x, int64_t ss, int64_t sc, int64_t S, int64_t C, int64_t D, const void* ws, int64_t bytes, int64_t key_bytes) {
  HTA_REQUIRE(x && S >= 4 && C >= 1 && D >= 1 && S < (1ll << 31) && D < (1ll << 31) && C < (1ll << 31) && S * C < (1ll << 31),
              "%s: bad shape (S=%lld C=%lld D=%lld): at least 4 draws, S C < 2^31", who, (long long)S, (long long)C, (long long)D);
  HTA_REQUIRE(sc >= D && ss >= (C - 1) * sc + D, "%s: bad strides (stride_s=%lld stride_c=%lld): rows and chains must not overlap", who, (long long)ss,
              (long long)sc);
  const DiagRankLayout L = diag_rank_layout(S * C, D, key_bytes);
  HTA_REQUIRE(D * L.nblk < (1ll << 31), "%s: bad shape (S C=%lld D=%lld): %lld tiles of %d keys are beyond one grid; pass fewer coordinates per call", who,
              (long long)(S * C), (long long)D, (long long)(D * L.nblk), DIAG_RANK_TILE);
  HTA_REQUIRE(ws && ((uintptr_t)ws & 7) == 0 && bytes >= L.total, "%s: workspace of %lld bytes (8-byte aligned) needed, %lld given", who, (long long)L.total,
              (long long)bytes);
  return HTA_OK;
}

// keys / payloads in (ka, ia) sorted by key, stably, through (kb, ib); an even number of passes: the result is in (ka, ia)
template <typename K>
static int diag_rank_sort(K* ka, uint32_t* ia, K* kb, uint32_t* ib, uint32_t* hist, uint32_t N, int64_t D, uint32_t nblk, hipStream_t st) {
  const unsigned grid = (unsigned)(D * nblk);
  note_route("diag_rank_scatter_kernel<uint%d>", (int)(8 * sizeof(K)));
  for (int pass = 0; pass < (int)sizeof(K); ++pass) {
    const int shift = 8 * pass;
    diag_rank_hist_kernel<K><<<grid, DIAG_RANK_THREADS, 0, st>>>(ka, N, nblk, shift, hist);
    HTA_CHECK_LAUNCH("diag_rank_hist_kernel");
    diag_rank_scan_kernel<<<(unsigned)D, DIAG_RANK_SCAN_THREADS, 0, st>>>(hist, nblk);
    HTA_CHECK_LAUNCH("diag_rank_scan_kernel");
    diag_rank_scatter_kernel<K><<<grid, DIAG_RANK_THREADS, 0, st>>>(ka, ia, kb, ib, N, nblk, shift, hist);
    HTA_CHECK_LAUNCH("diag_rank_scatter_kernel");
    K* tk = ka; ka = kb; kb = tk;
    uint32_t* ti = ia; ia = ib; ib = ti;
  }
  return HTA_OK;
}

template <typename T, typename K, bool FOLD>
static int diag_rank(const char* who, const T* x, int64_t ss, int64_t sc, int64_t S, int64_t C, int64_t D, const double* centre_in, double* z_out, float* i05_out,
                     float* i95_out, double* q05, double* median, double* q95, double* centre_out, int32_t* bad, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = diag_rank_check(who, x, ss, sc, S, C, D, workspace, workspace_bytes, sizeof(K))) return rc;
  HTA_REQUIRE(z_out && bad && (FOLD ? centre_in != nullptr : (i05_out && i95_out && q05 && median && q95 && centre_out)), "%s: an output pointer is NULL", who);
  const DiagRankLayout L = diag_rank_layout(S * C, D, sizeof(K));
  char* w = (char*)workspace;
  K *ka = (K*)(w + L.keys_a), *kb = (K*)(w + L.keys_b);
  uint32_t *ia = (uint32_t*)(w + L.idx_a), *ib = (uint32_t*)(w + L.idx_b), *hist = (uint32_t*)(w + L.hist);
  const uint32_t N = (uint32_t)(S * C), nblk = (uint32_t)L.nblk;
  const unsigned grid = (unsigned)(D * L.nblk);
  hipStream_t st = (hipStream_t)stream;
  if (!FOLD && hipMemsetAsync(bad, 0, sizeof(int32_t) * D, st) != hipSuccess) { set_error("%s: hipMemsetAsync failed", who); return HTA_ERR_LAUNCH; }
  diag_rank_gather_kernel<T, K, FOLD><<<grid, DIAG_RANK_THREADS, 0, st>>>(x, ss, sc, N, (uint32_t)C, nblk, centre_in, ka, ia, bad);
  HTA_CHECK_LAUNCH("diag_rank_gather_kernel");
  if (int rc = diag_rank_sort<K>(ka, ia, kb, ib, hist, N, D, nblk, st)) return rc;
  diag_rank_transform_kernel<K, !FOLD><<<grid, DIAG_RANK_THREADS, 0, st>>>(ka, ia, N, nblk, D, bad, z_out, i05_out, i95_out, q05, median, q95, centre_out);
  HTA_CHECK_LAUNCH("diag_rank_transform_kernel");
  return HTA_OK;
}

}  // namespace hta

extern "C" {

int hta_diag_rank_tile(void) { return hta::DIAG_RANK_TILE; }

double hta_diag_rank_ndtri(double p) { return hta::diag_ndtri(p); }

int64_t hta_diag_rank_workspace_bytes(int64_t S, int64_t C, int64_t D, int key_bytes) {
  if (S < 1 || C < 1 || D < 1 || (key_bytes != 4 && key_bytes != 8) || S >= (1ll << 31) || C >= (1ll << 31) || D >= (1ll << 31) || S * C >= (1ll << 31)) return -1;
  return hta::diag_rank_layout(S * C, D, key_bytes).total;
}

int hta_diag_rank_f32(const float* x, int64_t stride_s, int64_t stride_c, int64_t S, int64_t C, int64_t D, double* z, float* i05, float* i95, double* q05,
                      double* median, double* q95, double* centre, int32_t* bad, void* workspace, int64_t workspace_bytes, void* stream) {
  return hta::diag_rank<float, uint32_t, false>("hta_diag_rank", x, stride_s, stride_c, S, C, D, nullptr, z, i05, i95, q05, median, q95, centre, bad, workspace,
                                                workspace_bytes, stream);
}
int hta_diag_rank_f64(const double* x, int64_t stride_s, int64_t stride_c, int64_t S, int64_t C, int64_t D, double* z, float* i05, float* i95, double* q05,
                      double* median, double* q95, double* centre, int32_t* bad, void* workspace, int64_t workspace_bytes, void* stream) {
  return hta::diag_rank<double, uint64_t, false>("hta_diag_rank", x, stride_s, stride_c, S, C, D, nullptr, z, i05, i95, q05, median, q95, centre, bad, workspace,
                                                 workspace_bytes, stream);
}
int hta_diag_rank_folded_f32(const float* x, int64_t stride_s, int64_t stride_c, int64_t S, int64_t C, int64_t D, const double* centre, double* zf, int32_t* bad,
                             void* workspace, int64_t workspace_bytes, void* stream) {
  return hta::diag_rank<float, uint64_t, true>("hta_diag_rank_folded", x, stride_s, stride_c, S, C, D, centre, zf, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               bad, workspace, workspace_bytes, stream);
}
int hta_diag_rank_folded_f64(const double* x, int64_t stride_s, int64_t stride_c, int64_t S, int64_t C, int64_t D, const double* centre, double* zf, int32_t* bad,
                             void* workspace, int64_t workspace_bytes, void* stream) {
  return hta::diag_rank<double, uint64_t, true>("hta_diag_rank_folded", x, stride_s, stride_c, S, C, D, centre, zf, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                bad, workspace, workspace_bytes, stream);
}

}  // extern "C"
