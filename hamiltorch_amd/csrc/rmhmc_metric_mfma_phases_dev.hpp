// Matrix-core metric kernel: the out-of-line phases (ph_*) of the general sequence - staging, log p, the refinement's element-wise
// passes, the triangular solves, the derivative matrix.  The sequence itself (metric_warm_system) is in rmhmc_metric_mfma_general_dev.hpp.
#pragma once
#include "rmhmc_metric_mfma_vec_dev.hpp"

namespace hta {

constexpr float kFallbackE = 0.03f;   // max |E_ij| beyond which the refinement is not trusted
constexpr float kConvE = 3e-4f;       // an update with max |E_ij| below this leaves an error of order 1e-7
constexpr float kSecondE = 8e-3f;     // a first pass with max |E_ij| below this is followed by the second-order pass (ph_refine_E2): its
                                      // truncation leaves ||A X - X Lam|| of order |F| d^2 (d = max |E_ij|): < 1e-8 here, below fp32 rounding


// ---- the phases of an evaluation, each OUT OF LINE ---------------------------------------------------------------------
// Inlined into one kernel body, the compiler hoists every phase's per-thread address arithmetic over the whole kernel and
// keeps it alive across the others: > 128 live registers at 1024 threads, i.e. scratch traffic inside the loops.  As
// functions nothing is live across a phase but a few scalars.  LDS operands are offsets (see lds_gemm); global operands
// are cast back to the global address space (a generic pointer argument would become flat loads).
typedef const __attribute__((address_space(1))) float* gcf;
#define HTA_LDS_BASE() extern __shared__ __attribute__((aligned(16))) char smem_raw[]; float* const lds = reinterpret_cast<float*>(smem_raw)
#define HTA_U(x) __builtin_amdgcn_readfirstlane(x)

__device__ HTA_PH_ATTR void jacobi_fallback(int offA, int offVT, int D, int ne, int LD, int offCs, int offRed, int max_sweeps) {
  HTA_LDS_BASE();
  D = HTA_U(D); ne = HTA_U(ne); LD = HTA_U(LD); max_sweeps = HTA_U(max_sweeps);
  lds_jacobi<float, 2, 2>(lds + HTA_U(offA), lds + HTA_U(offVT), D, ne, LD, LD, lds + HTA_U(offCs), nullptr, lds + HTA_U(offRed), max_sweeps);
}

__device__ HTA_PH_ATTR void ph_stage(const float* src, int offDst, int D, int DP, int LD) {
  HTA_LDS_BASE();
  stage_dense((gcf)src, lds + HTA_U(offDst), HTA_U(D), HTA_U(DP), HTA_U(LD));
}

// sum_i d_i (P d)_i over the block, upd_g += cg P d  (d in LDS at offVd; P symmetric, global)
__device__ HTA_PH_ATTR float ph_logp(const float* P, int offVd, int D, int offPart, int offRed, float* upd_g, float cg) {
  HTA_LDS_BASE();
  D = HTA_U(D);
  const float* vd = lds + HTA_U(offVd);
  const float pd = gmv_sym((gcf)P, vd, D, lds + HTA_U(offPart));
  float part = 0.f;
  if ((int)threadIdx.x < D) {
    part = vd[threadIdx.x] * pd;
    if (upd_g) { __attribute__((address_space(1))) float* g = (__attribute__((address_space(1))) float*)upd_g; g[threadIdx.x] += cg * pd; }
  }
  return block_sum_dpp(part, lds + HTA_U(offRed));
}

// M (or M^T) v with M [n][ld] and v in LDS; every lane of row (tid >> 3)'s group of 8 returns the row's sum
__device__ HTA_PH_ATTR float ph_mv8(int trans, int offM, int ld, int offV, int n) {
  HTA_LDS_BASE();
  ld = HTA_U(ld); n = HTA_U(n);
  const float* M = lds + HTA_U(offM); const float* v = lds + HTA_U(offV);
  return HTA_U(trans) ? mv8<true>(M, ld, v, n) : mv8<false>(M, ld, v, n);
}

// One pass of the refinement's element-wise step: lam_i = S_ii / Gm_ii, then E from S (at offS) and Gm (at offG; the
// identity when have_x == 0) into offDst (which may be offS).  Returns max |E_ij|, i != j (1 for NaN / inf / > kFallbackE).
__device__ HTA_PH_ATTR float ph_refine_E(int offS, int offG, int offDst, int offLam, int offRed, int have_x, int D, int LD) {
  HTA_LDS_BASE();
  D = HTA_U(D); LD = HTA_U(LD); have_x = HTA_U(have_x);
  const float* by = lds + HTA_U(offS); const float* bz = lds + HTA_U(offG);
  float* edst = lds + HTA_U(offDst); float* vlam = lds + HTA_U(offLam); float* red = lds + HTA_U(offRed);
  const int tid = threadIdx.x;
  float scale = 0.f;
  if (tid < D) {
    const float l = have_x ? by[tid * LD + tid] / bz[tid * LD + tid] : by[tid * LD + tid];
    vlam[tid] = l;
    scale = fabsf(l);
  }
  scale = block_max(scale, red);                                   // (its barriers also publish vlam)
  const float tiny = 8.f * Eps<float>::v * scale;
  float emax = 0.f;
  // The off-diagonal elements in PAIRS (i, j), (j, i), i < j: S and Gm are symmetric (the products mirror their upper tiles), the
  // two quotients share the reciprocal of lam_j - lam_i.  Row r and row D - 1 - r have D - 1 upper elements between them: the
  // pairs form a [ceil(D / 2)][D - 1] rectangle - thread (c = tid & 127, r = tid >> 7 + 8 p) needs no index division.
  // (Rounds 2-3 walked all D^2 elements, a division each: 12.8 k + 10.7 k of an evaluation's 108 k cycles.)
  const int c = tid & 127, H = (D + 1) >> 1;
  if (tid < D) {                                                   // the diagonal: E_ii = (1 - Gm_ii) / 2 (+ 1: the first pass writes X = I + E)
    const float gm = have_x ? bz[tid * LD + tid] : 1.f;
    edst[tid * LD + tid] = 0.5f * (1.f - gm) + (have_x ? 0.f : 1.f);
  }
#pragma unroll
  for (int p8 = 0; p8 < 7; ++p8) {
    const int r = (tid >> 7) + 8 * p8;
    if (r >= H || c >= D - 1) continue;
    const int n1 = D - 1 - r;
    int i, j;
    if (c < n1) { i = r; j = r + 1 + c; }
    else { i = D - 1 - r; j = D - r + (c - n1); if (i == r) continue; }          // (odd D: the middle row is its own partner)
    const float li = vlam[i], lj = vlam[j];
    const float sij = by[i * LD + j];
    const float gm = have_x ? bz[i * LD + j] : 0.f;
    const float rinv = __builtin_amdgcn_rcpf(lj - li);
    const float nu = sij - lj * gm, nl = sij - li * gm;
    const float eu = (fabsf(nu) <= tiny) ? -0.5f * gm : nu * rinv;                // E_ij = (S_ij - lam_j Gm_ij) / (lam_j - lam_i)
    const float el = (fabsf(nl) <= tiny) ? -0.5f * gm : -(nl * rinv);             // E_ji = (S_ij - lam_i Gm_ij) / (lam_i - lam_j)
    const float em = fmaxf(fabsf(eu), fabsf(el));
    emax = fmaxf(emax, em);
    if (!(fabsf(eu) <= kFallbackE) || !(fabsf(el) <= kFallbackE)) emax = 1.f;     // NaN / inf / too large
    edst[i * LD + j] = eu;
    edst[j * LD + i] = el;
  }
  return block_max(emax, red);
}

// The SECOND pass in closed form (round 4).  After the first pass X = I + E1 with E1 antisymmetric (the pairs above) and zero on the
// diagonal, the refinement's quantities are, up to terms of third order in the perturbation F = A - diag(A):
//     S_ij - lam_j Gm_ij = (F E1)_ij =: M_ij  (i != j),    lam_i' = S_ii / Gm_ii = lam_i + M_ii,    Gm_ii = 1 + sum_k E1_ki^2
// (the first-order terms cancel by the choice of E1; (E1^T Lam E1 - lam_j E1^T E1)_ij = -(E1^T F)_ij cancels one of the two
// mixed terms) - i.e. second-order perturbation theory: ONE full product M = F E1 instead of T = A X, S = X^T T and Gm = X^T X
// (2.1 full products), with E2_ij = M_ij / (lam_j' - lam_i'), E2_ii = -1/2 sum_k E1_ki^2.  The caller zeroed the diagonals of A and
// X before the product; this pass reads M (offM) and E1 (offX, whose unit diagonal it restores), writes E2 to offDst, E2^T in M's
// place (a pair owns its two entries of M: the solve then reads both E2 and E2^T row-wise) and the corrected eigenvalues to offLam.  Returns max |E2_ij| (1 for NaN / inf / > kFallbackE).  Truncation: |A X2 - X2 Lam'| ~ |F| d^2.
__device__ HTA_PH_ATTR float ph_refine_E2(int offM, int offX, int offDst, int offLam, int offRed, int D, int LD) {
  HTA_LDS_BASE();
  D = HTA_U(D); LD = HTA_U(LD);
  float* M = lds + HTA_U(offM); float* X = lds + HTA_U(offX);
  float* edst = lds + HTA_U(offDst); float* vlam = lds + HTA_U(offLam); float* red = lds + HTA_U(offRed);
  const int tid = threadIdx.x;
  float scale = 0.f;
  {
    const int row = tid >> 3, seg = tid & 7;                       // sum_k E1_ki^2 = sum_k E1_ik^2: 8 lanes per row
    float c0 = 0.f, c1 = 0.f;
    if (row < D) {
#pragma unroll
      for (int u = 0; u < 14; ++u) {
        const int k = seg + 8 * u;
        const float v = k < D ? X[row * LD + k] : 0.f;
        if (u & 1) c1 = fmaf(v, v, c1); else c0 = fmaf(v, v, c0);
      }
    }
    float cs = c0 + c1;
    cs = sum8_dpp(cs);
    if (seg == 0 && row < D) {
      const float l2 = vlam[row] + M[row * LD + row];
      vlam[row] = l2;
      scale = fabsf(l2);
      edst[row * LD + row] = -0.5f * cs;
      M[row * LD + row] = -0.5f * cs;
      X[row * LD + row] = 1.f;
    }
  }
  scale = block_max(scale, red);                                   // (its barriers also publish vlam)
  // M is a product of small factors, not a difference of large ones: its rounding noise is RELATIVE (eps |F| d per term), far below
  // the full pass's threshold 8 eps |lam| on S_ij - lam_j Gm_ij (which would zero M itself: |M_ij| ~ 1e-6 at BASELINE config 3)
  const float tiny = 8.f * Eps<float>::v * scale * kSecondE;
  float emax = 0.f;
  const int c = tid & 127, H = (D + 1) >> 1;
#pragma unroll
  for (int p8 = 0; p8 < 7; ++p8) {
    const int r = (tid >> 7) + 8 * p8;
    if (r >= H || c >= D - 1) continue;
    const int n1 = D - 1 - r;
    int i, j;
    if (c < n1) { i = r; j = r + 1 + c; }
    else { i = D - 1 - r; j = D - r + (c - n1); if (i == r) continue; }
    const float rinv = __builtin_amdgcn_rcpf(vlam[j] - vlam[i]);
    const float nu = M[i * LD + j], nl = M[j * LD + i];
    const float eu = (fabsf(nu) <= tiny) ? 0.f : nu * rinv;
    const float el = (fabsf(nl) <= tiny) ? 0.f : -(nl * rinv);
    emax = fmaxf(emax, fmaxf(fabsf(eu), fabsf(el)));
    if (!(fabsf(eu) <= kFallbackE) || !(fabsf(el) <= kFallbackE)) emax = 1.f;
    edst[i * LD + j] = eu;
    edst[j * LD + i] = el;
    M[i * LD + j] = el;                                            // E2^T
    M[j * LD + i] = eu;
  }
  return block_max(emax, red);
}

__device__ HTA_PH_ATTR void ph_chol_solve(int offG, int D, int LD, int offV) {
  HTA_LDS_BASE();
  lds_chol_solve<float>(lds + HTA_U(offG), HTA_U(D), HTA_U(LD), lds + HTA_U(offV));
}

__device__ HTA_PH_ATTR float ph_mv8_lower(int offM, int ld, int offV, int n) {
  HTA_LDS_BASE();
  return mv8_lower(lds + HTA_U(offM), HTA_U(ld), lds + HTA_U(offV), HTA_U(n));
}

// a zero-padded [DP][LD] copy of the symmetric matrix whose LOWER triangle is in global memory (eigh UPLO = 'L', S:119), jitter
// (LDS vector at offJit) added on the diagonal
__device__ HTA_PH_ATTR void ph_stage_sym(const float* src, int offDst, int offJit, int D, int DP, int LD) {
  HTA_LDS_BASE();
  D = HTA_U(D); DP = HTA_U(DP); LD = HTA_U(LD);
  float* dst = lds + HTA_U(offDst); const float* vj = lds + HTA_U(offJit);
  gcf g = (gcf)src;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float v[7];
    const int j = lane + 64 * h;
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      const int i = wave + 16 * t;
      v[t] = (i < D && j < D) ? (i >= j ? g[i * D + j] : g[j * D + i]) : 0.f;
    }
#pragma unroll
    for (int t = 0; t < 7; ++t) { const int i = wave + 16 * t; if (i < DP && j < LD) dst[i * LD + j] = v[t] + ((i == j && i < D) ? vj[i] : 0.f); }
  }
}

// [D][D] row-major global <- the leading block of an LDS matrix
__device__ HTA_PH_ATTR void ph_store_dense(float* dstg, int offSrc, int D, int LD) {
  HTA_LDS_BASE();
  D = HTA_U(D); LD = HTA_U(LD);
  const float* src = lds + HTA_U(offSrc);
  __attribute__((address_space(1))) float* g = (__attribute__((address_space(1))) float*)dstg;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < D; i += MT / 64)
    for (int j = lane; j < D; j += 64) g[i * D + j] = src[i * LD + j];
}

// W of the derivative matrix M = Q W Q^T (HtaMetricArgs::dmetric_out; the same formula as metric_eval_kernel):
// W_kl = 1/2 [k == l] lam~'_k / lam~_k - 1/2 J_kl u_k u_l,  J = divided differences of lam -> lam~, zero padded
__device__ HTA_PH_ATTR void ph_dmetric_w(int offDst, int offLam, int offLt, int offU, float alpha, int D, int DP, int LD) {
  HTA_LDS_BASE();
  D = HTA_U(D); DP = HTA_U(DP); LD = HTA_U(LD);
  float* dst = lds + HTA_U(offDst);
  const float* vlam = lds + HTA_U(offLam); const float* vlt = lds + HTA_U(offLt); const float* vu = lds + HTA_U(offU);
  const int l = threadIdx.x & 127;
  for (int k = threadIdx.x >> 7; k < DP; k += MT / 128) {
    if (l >= LD) continue;
    float w = 0.f;
    if (k < D && l < D) {
      const float lk = vlam[k], ll = vlam[l], dl = lk - ll;
      float J;
      if (k == l || fabsf(dl) <= 1e-3f * (fabsf(lk) + fabsf(ll))) J = softabs_slope<float>(alpha, 0.5f * (lk + ll));
      else J = (vlt[k] - vlt[l]) / dl;
      w = -0.5f * J * vu[k] * vu[l];
      if (k == l) w += 0.5f * softabs_slope<float>(alpha, lk) / vlt[k];
    }
    dst[k * LD + l] = w;
  }
}

}  // namespace hta
