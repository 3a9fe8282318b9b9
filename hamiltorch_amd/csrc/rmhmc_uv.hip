// Explicit RMHMC for a Gaussian target on the identity-soft-abs path (see rmhmc_fused.hip for why that path exists and what
// it computes: hamiltorch/samplers.py:969-1026 with the integrator S:425-461; its launcher, rmhmc_fused_sample, hands over to
// rmhmc_uv_launch below, and the one-chain VALU kernel these are measured against is rmhmc_fused_chain_dev.hpp's), ONE or TWO chains per workgroup on the matrix
// cores, for every chain count up to 2 x (compute units): rmhmc_uv_kernel<G, CO>, and the dispatch to its successors in
// rmhmc_uvc.hip (rmhmc_uvc_kernel: one-chain groups with K == 2 and jitter; rmhmc_uvc2_kernel: two-chain groups), which leaves
// this kernel the one-chain groups without jitter or with K != 2.
//
// The trajectory, the step (cols_steps: 5 phases and 312 matrix instructions per wave at K = 2; the one-chain VALU kernel: 8
// phases, 896 v_fmac_f32_dpp per lane at about 9 clocks each) and the Hamiltonian are those of rmhmc_cols_dev.hpp; UvTile is this
// kernel's layout: the product leaves four rows per lane, and lane (row block, column) keeps ITS set's four rows - at both
// contraction parities, which hold bit-identical duplicates ("duplicate state, one writer").
#include <math.h>
#include "rmhmc_cols_dev.hpp"

namespace hta {

// These kernels run one wave per SIMD: nothing hides an instruction of the element-wise / bookkeeping stretches between their
// matrix phases ("what comes next"), so (measured: profiles/r03y_ab_lines.txt) (i) put has no lane predicate: both
// parities store - same address, same value - and the s_and_saveexec / s_cbranch_execz / s_or_b64 around every store go;
// (ii) the padding rows (>= D) of every state vector are exact zeros by construction (zero matrix rows, zero jitter, zero mu_r),
// so X - mu needs no select there.  A chain that went non-finite may carry NaN into its own padding rows; it is rejected, and
// every vector is rewritten from the clean current point before the next trajectory reads it.
template <int G> struct UvTile : ColsLane {
  static constexpr int NV = 4, NC = G, NBUF = 9;       // LDS vector matrices: DV GV EV W0 W1 + 4 solve buffers [pair][iteration parity]
  typedef float bf2 __attribute__((ext_vector_type(2)));
  T *WS, *red;                     // half steps: refinement vectors | [XWV][XNC][4]
  int cidx, own_off, row[4];
  bool rok[4], lead, writer, row_writer;
  T mu_r[4], sd_r[4];

  __device__ __forceinline__ UvTile(const FusedArgs<float>& a_, T* lds) : ColsLane(a_, lds) {
    WS = W0 + 2 * MSZ; red = WS + 4 * MSZ;
    cidx = cl >> 1; lead = (l >> 2) == 0;
    writer = !setV && w == 0 && lead; row_writer = !khi && !setV;
#pragma unroll
    for (int e = 0; e < 4; ++e) {                         // this lane OWNS rows row0..row0+3 of its column
      row[e] = row0 + e;
      rok[e] = row[e] < a.D;
      mu_r[e] = rok[e] ? a.mu[row[e]] : 0.f;
      sd_r[e] = rok[e] ? a.S[(int64_t)row[e] * a.D + row[e]] : 0.f;
    }
    zero_lds(NBUF * MSZ + XWV * XNC * 4);
    own_off = cl * XLD + (row0 >> 1);                     // rows row0, row0+2 -> even half; row0+1, row0+3 -> odd half
  }
  __device__ __forceinline__ void put(T* X, const T (&v)[4]) const {
    *reinterpret_cast<bf2*>(X + own_off) = bf2{v[0], v[2]};
    *reinterpret_cast<bf2*>(X + own_off + XHL) = bf2{v[1], v[3]};
  }
  __device__ __forceinline__ void extract(const bf4& acc, T (&v)[4]) const {   // lanes l and l ^ 8 both end with (even k) + (odd k)
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = acc[e] + other_parity(acc[e]);
  }
  __device__ __forceinline__ T dot(const T (&x)[4], const T (&y)[4]) const {
    T s = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) s += x[e] * y[e];
    return s;
  }
  // three sums per column over the rows, complete in every lane of the column (the odd parity holds duplicates: it adds nothing)
  __device__ __forceinline__ void sums(T (&v)[3]) const {
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      if (khi) v[e] = 0.f;
      v[e] += __shfl_xor(v[e], 4, 64);
      v[e] += __shfl_xor(v[e], 16, 64);
      v[e] += __shfl_xor(v[e], 32, 64);
    }
    __syncthreads();
    if (lead) {
#pragma unroll
      for (int e = 0; e < 3; ++e) red[(w * XNC + cl) * 4 + e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      T s = 0.f;
#pragma unroll
      for (int i = 0; i < XWV; ++i) s += red[(i * XNC + cl) * 4 + e];
      v[e] = s;
    }
  }
  // the jitter of this lane's four rows for one sub-stream (uniform_elem layout: rows 4b..4b+3 are Philox block b)
  __device__ __forceinline__ void jitter_one(uint32_t n, uint32_t sub, T (&out)[4]) const {
    const U4 r = philox_block(a.seed, chain, n, PURPOSE_JITTER, sub, (uint32_t)(row0 >> 2));
    const T u[4] = {u23<T>(r.x), u23<T>(r.y), u23<T>(r.z), u23<T>(r.w)};
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = (live && rok[e]) ? a.jitter * u[e] : 0.f;
  }
  // The even parity draws this column's block of the first pair, the odd parity that of the second pair, then they exchange:
  // one Philox pass per step and lane (about 1000 clocks of a 9000-clock step).  Measured and rejected (profiles/README.md,
  // r02r - r02t): the pass's rounds issued one per chunk of eight matrix instructions of the refresh phase - 1.5x SLOWER
  // (3.08e7 against 4.71e7 steps/s at 256 chains: a wave issues in order, a quarter-rate multiply holds back the matrix
  // instructions behind it); one round in each window where a phase waits for LDS (after the operand fetch, between the stores
  // and the barrier) - 5 % slower.
  __device__ __forceinline__ void jitter_pair(uint32_t n, uint32_t subA, uint32_t subB, T (&eA)[4], T (&eB)[4]) const {
    T mine[4];
    jitter_one(n, khi ? subB : subA, mine);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const T oth = other_parity(mine[e]);
      eA[e] = khi ? oth : mine[e];
      eB[e] = khi ? mine[e] : oth;
    }
  }
  // the set that moves first in S:429-433 is U, in S:454-458 (second) V: it kicks before its solve, the other one after
  __device__ __forceinline__ void kick(bool second, bool after, const T (&X)[4], T (&g)[4], const T (&y)[4], T (&z)[4]) const {
    const bool first = second ? setV : !setV;
    if (first != after) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        g[i] -= eh * y[i];
        z[i] -= eh * (X[i] - mu_r[i]);
      }
    }
  }
  __device__ __forceinline__ void steps(uint32_t n, T (&X)[4], T (&g)[4], T (&y)[4], T (&z)[4]) { cols_steps(*this, n, X, g, y, z); }
  __device__ __forceinline__ void hamiltonian(uint32_t n, uint32_t sub, const T (&X)[4], const T (&g)[4], T& H, T& logp, T (&Pd)[4],
                                              T (&Sg)[4], T& kin, T& ld) {
    cols_hamiltonian(*this, n, sub, X, g, H, logp, Pd, Sg, kin, ld);
  }
};

// CO (tuning key "rmhmc_uv_co", default 1): the same code under a 256-register cap, so that TWO workgroups share a CU (one wave
// of each per SIMD): a phase is a latency chain (LDS publish - barrier - operand fetch - 52 dependent matrix instructions -
// combine) that leaves the matrix pipe idle more than half of the time; a second, independent workgroup fills those gaps.  The
// capped build keeps S and P in VGPRs (no accumulation registers at all: the matrix instructions write VGPRs directly) and
// spills nothing inside the step loop (tests/test_kernel_resources.py).
template <int G, bool CO>                                  // chains per workgroup
__global__ __launch_bounds__(XNT, CO ? 2 : 1) void rmhmc_uv_kernel(FusedArgs<float> a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  UvTile<G> t(a, reinterpret_cast<float*>(smem_raw));
  cols_trajectories(a, t);
}

int g_rmhmc_uv = 1;          // rmhmc_uv.hip (one or two chains per workgroup as columns of the matrix instruction): 1 up to 2 x CUs chains, 0 off, 2 always
int g_rmhmc_uv_co = 1;       // tuning key "rmhmc_uv_co" (default 1): the 256-register instances, two workgroups per CU; 0 = the uncapped ones
int g_rmhmc_uv_g = 0;        // tuning key "rmhmc_uv_g": chains per workgroup (0 = by chain count, 1, 2)

int rmhmc_uv_launch(const FusedArgs<float>& a, int cus, hipStream_t s) {
  const size_t bytes = (size_t)(UvTile<1>::NBUF * XNC * XLD + XWV * XNC * 4) * sizeof(float);
  const int g = g_rmhmc_uv_g == 1 || g_rmhmc_uv_g == 2 ? g_rmhmc_uv_g : (a.C <= cus ? 1 : 2);
  const int64_t ngroup = (a.C + g - 1) / g;
  const int grid = (int)(ngroup < 8192 ? ngroup : 8192);
  const bool co = g_rmhmc_uv_co != 0;
  if (g == 1 && g_rmhmc_uvc && a.K == 2 && a.has_jitter) return rmhmc_uvc_launch(a, co, s);
  // (round 5, measured and not kept - tools/scratch/rmhmc_uvc2d.hip.rejected, profiles/r05b_uvc2d_ab.txt: the one-chain kernel's three
  //  phases per step for two-chain groups, the deferred second-order products as extra accumulator chains: 364 matrix instructions and 3
  //  barriers per step instead of 312 and 5, equal to rounding - 5 % SLOWER at 1024 chains (4.64 against 4.39 ms), slower at 384 ... 1536:
  //  with two workgroups per CU the phases' latency is already covered, the extra matrix instructions are not)
  if (g == 2 && g_rmhmc_uvc) return rmhmc_uvc2_launch(a, co, s);
  note_route("rmhmc_uv_kernel<%d,%s>", g, co ? "co" : "solo");
  if (g == 1) {
    if (co) rmhmc_uv_kernel<1, true><<<grid, XNT, bytes, s>>>(a);
    else rmhmc_uv_kernel<1, false><<<grid, XNT, bytes, s>>>(a);
  } else {
    if (co) rmhmc_uv_kernel<2, true><<<grid, XNT, bytes, s>>>(a);
    else rmhmc_uv_kernel<2, false><<<grid, XNT, bytes, s>>>(a);
  }
  return HTA_OK;
}

}  // namespace hta
