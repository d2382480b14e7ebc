// Cholesky form of the global stage's orthogonalisation (R > frames): C = M^T G M (pmd_gram_mtgm), its blocked
// factorisation and the inverse factor (pmd_chol_inverse, pmd_orthogonalize_chol).  Matrices are row-major; the rocBLAS /
// rocSOLVER calls see the row-major lower triangle as the column-major upper one.
#include "pmd_internal.h"
#include <rocsolver/rocsolver.h>
#include <algorithm>
#include <cmath>

// =============================================================================================
// Cholesky form of the orthogonalisation (R > frames): any P with the column space of `right` and
// P^T G P = I gives the same final R, s, Vt (P_chol = P_eigh Q with Q orthogonal, and the
// projected SVD absorbs Q).  C = M^T G M = U_c^T U_c (upper Cholesky), P = M U_c^{-1}, i.e.
// Et = U_c^{-T} (lower triangular).  ok_host = 0 when C is not numerically positive definite
// (the caller then uses the eigendecomposition, decomposition.py:984-996).
// =============================================================================================
// Cholesky factor of one diagonal block (nb <= 128): A = L L^T, row-major lower triangle in place.
// One workgroup of 16 x 16 threads; thread (tr, tc) keeps the entries r = tr (mod 16), c = tc (mod 16) in
// registers for the whole factorisation, only the pivot column travels through LDS (one barrier per step).
// *info = 1-based global index of the first non-positive pivot (left untouched otherwise).
#define CHOL_NB 128
// n_abs_last > 0: a negative pivot number n_abs_last (1-based, the LAST pivot of the whole matrix) is replaced by its
// absolute value - the Cholesky-route form of the reference keeping a numerically null direction through |lambda|.
#define CHOL_LS (CHOL_NB + 1)
__global__ __launch_bounds__(256) void potf2_block_kernel(float* __restrict__ A, long ld, int nb, int k0, int* __restrict__ info,
                                                          int n_abs_last) {
  __shared__ float s_col[2][CHOL_NB];
  const int tid = threadIdx.x;
  const int tr = tid >> 4, tc = tid & 15;
  float a[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = tr + 16 * i, c = tc + 16 * j;
      const bool in = r < nb && c <= r;
      const float v = A[(long)(in ? r : 0) * ld + (in ? c : 0)];  // unconditional load, masked value
      a[i][j] = in ? v : 0.f;
    }
  int bad = 0;
  for (int k = 0; k < nb; ++k) {
    float* col = s_col[k & 1];
    const int jk = k >> 4;
    if (tc == (k & 15)) {
      // this thread owns entries of column k: publish the part on and below the diagonal
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int r = tr + 16 * i;
        float v = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) v = (j == jk) ? a[i][j] : v;
        if (r >= k && r < nb) col[r] = v;
      }
    }
    __syncthreads();
    float piv = col[k];
    if (!(piv > 0.f)) {
      if (k0 + k + 1 == n_abs_last && piv < 0.f) {
        piv = -piv;
      } else {
        bad = k0 + k + 1;
        break;  // uniform: every thread reads the same pivot
      }
    }
    const float dk = sqrtf(piv);
    const float inv = 1.f / dk;
    float lr[8], lc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = tr + 16 * i, c = tc + 16 * i;
      const float vr = col[r], vc = col[c];  // unconditional LDS reads (stale entries above the pivot are masked)
      lr[i] = (r > k && r < nb) ? vr * inv : 0.f;
      lc[i] = (c > k && c < nb) ? vc * inv : 0.f;
    }
    // only register columns j >= k / 16 and rows i >= j can still change (uniform tests: whole slabs are skipped)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j < jk) continue;
#pragma unroll
      for (int i = j; i < 8; ++i) {
        const int r = tr + 16 * i, c = tc + 16 * j;
        // trailing update (c > k, r >= c): lr, lc are zero outside it except for r < c, which is masked here
        if (r >= c) a[i][j] -= lr[i] * lc[j];
        // column k itself: the scaled entries and the pivot
        if (j == jk && c == k) a[i][j] = (r == k) ? dk : ((r > k) ? lr[i] : a[i][j]);
      }
    }
  }
  if (bad) {
    if (tid == 0 && *info == 0) *info = bad;
    return;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = tr + 16 * i, c = tc + 16 * j;
      if (r < nb && c <= r) A[(long)r * ld + c] = a[i][j];
    }
}

// Panel of the blocked factorisation, in place: P (rest x nb, row-major, leading dimension ld) <- P L^{-T}, with
// linv = row-major L^{-1} (leading dimension CHOL_NB); a compact copy (leading dimension CHOL_NB) feeds the trailing update.
// 16 rows per workgroup; the inverse passes through LDS in four slabs of 32 inner indices, transposed on the way in.
// 25 KB of LDS: the chain runs next to large products on the main stream, and a workgroup that asks for more than the
// CU has left waits for one of theirs to retire (measured: a 83 KB version of this kernel and a 132 KB fused
// factor-and-invert kernel were faster alone and 11 ms slower in the step).
// (rocBLAS picks 16 x 16 / 128 x 64 macro tiles for this 128-deep product: 130-180 us per panel.)
#define CHOL_PR 16
__global__ __launch_bounds__(256) void chol_panel_kernel(float* __restrict__ P, long ld, int rest, int nb, const float* __restrict__ linv,
                                                         float* __restrict__ compact) {
  __shared__ float Ps[CHOL_PR][CHOL_LS];
  __shared__ float Lt[32][CHOL_LS];            // Lt[k - k0][j] = linv[j][k]
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * CHOL_PR;
  for (int idx = tid; idx < CHOL_PR * CHOL_NB; idx += 256) {
    const int r = idx / CHOL_NB, k = idx - r * CHOL_NB;
    Ps[r][k] = (r0 + r < rest && k < nb) ? P[(long)(r0 + r) * ld + k] : 0.f;
  }
  const int ty = tid >> 5, tx = tid & 31;   // rows 2 ty, 2 ty + 1; columns tx + 32 q
  float acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  for (int k0 = 0; k0 < nb; k0 += 32) {
    __syncthreads();
    for (int idx = tid; idx < CHOL_NB * 32; idx += 256) {
      const int j = idx >> 5, kk = idx & 31;
      Lt[kk][j] = (j < nb && k0 + kk <= j) ? linv[(long)j * CHOL_NB + k0 + kk] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < 32; ++kk) {
      const float p0 = Ps[2 * ty][k0 + kk], p1 = Ps[2 * ty + 1][k0 + kk];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float lv = Lt[kk][tx + 32 * b];
        acc[0][b] += p0 * lv;
        acc[1][b] += p1 * lv;
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int r = r0 + 2 * ty + a;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = tx + 32 * b;
      if (r < rest && j < nb) {
        P[(long)r * ld + j] = acc[a][b];
        compact[(long)r * CHOL_NB + j] = acc[a][b];
      }
    }
  }
}

// Blocked right-looking Cholesky of the row-major lower triangle (= column-major upper, A = U^T U):
// diagonal block in LDS, panel by rocBLAS strsm, trailing update by ssyrk.  rocSOLVER's spotrf spends half
// of its 35 ms at n = 10^4 in its unblocked diagonal-block kernel.
// tmp: n x CHOL_NB floats (the panel before it is copied back), linv: CHOL_NB x CHOL_NB floats
static int chol_lower_rm(pmd_ctx* ctx, int n, float* A, long ld, int* info, float* tmp, float* linv, int abs_last_pivot) {
  pmd_prof_scope prof__(ctx, "cholesky");
  PMD_HIP(ctx, hipMemsetAsync(info, 0, sizeof(int), ctx->stream));
  // (belt and braces: strtri writes the whole block, zeros in the other triangle included, and chol_panel_kernel masks that
  // triangle; no result depends on this clear)
  PMD_HIP(ctx, hipMemsetAsync(linv, 0, sizeof(float) * CHOL_NB * CHOL_NB, ctx->stream));
  const float one = 1.f, minus1 = -1.f;
  // PMD_CHOL_CHAIN=rocblas: the earlier chain (strtri on the block, panel by sgemm into a copy) for A/B runs
  const bool own_chain = !ctx->routes.chol_chain_rocblas;
  for (int k0 = 0; k0 < n; k0 += CHOL_NB) {
    const int nb = std::min(CHOL_NB, n - k0);
    float* D = A + (long)k0 * ld + k0;
    const int rest = n - k0 - nb;
    hipLaunchKernelGGL(potf2_block_kernel, dim3(1), dim3(256), 0, ctx->stream, D, ld, nb, k0, info, abs_last_pivot ? n : -1);
    PMD_LAUNCH_CHECK(ctx, "potf2_block_kernel");
    if (rest <= 0) break;
    float* P = A + (long)(k0 + nb) * ld + k0;        // row-major rest x nb  ==  column-major nb x rest
    float* T22 = A + (long)(k0 + nb) * ld + (k0 + nb);
    // L21 = A21 L_kk^{-T}: invert the 128 x 128 block (column-major upper view of the row-major lower block)
    // and multiply - rocBLAS' strsm spends ~20 small launches per panel on the same thing
    PMD_BLAS(ctx, rocblas_strtri(ctx->blas, rocblas_fill_upper, rocblas_diagonal_non_unit, nb, D, (rocblas_int)ld, linv, CHOL_NB));
    if (own_chain) {
      // in place (+ a compact copy for the trailing update)
      hipLaunchKernelGGL(chol_panel_kernel, dim3((rest + CHOL_PR - 1) / CHOL_PR), dim3(256), 0, ctx->stream, P, ld, rest, nb, linv, tmp);
      PMD_LAUNCH_CHECK(ctx, "chol_panel_kernel");
      PMD_BLAS(ctx, rocblas_ssyrk(ctx->blas, rocblas_fill_upper, rocblas_operation_transpose, rest, nb, &minus1, tmp, CHOL_NB, &one,
                                  T22, (rocblas_int)ld));
      continue;
    }
    RUN(pmd_gemm_rm(ctx, 0, 1, rest, nb, nb, 1.f, P, ld, linv, CHOL_NB, 0.f, tmp, CHOL_NB));
    PMD_HIP(ctx, hipMemcpy2DAsync(P, (size_t)ld * sizeof(float), tmp, (size_t)CHOL_NB * sizeof(float), (size_t)nb * sizeof(float),
                                  rest, hipMemcpyDeviceToDevice, ctx->stream));
    PMD_BLAS(ctx, rocblas_ssyrk(ctx->blas, rocblas_fill_upper, rocblas_operation_transpose, rest, nb, &minus1, tmp,
                                CHOL_NB, &one, T22, (rocblas_int)ld));
  }
  return PMD_OK;
}

__global__ void tril_mask_kernel(float* __restrict__ A, long ld, int n) {
  const int i = blockIdx.y;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x)
    if (j > i) A[(long)i * ld + j] = 0.f;
}

extern "C" size_t pmd_orthogonalize_chol_workspace_bytes(int Rc, int m) {
  return std::max(pmd_gram_mtgm_workspace_bytes(Rc, m), pmd_chol_inverse_workspace_bytes(m)) + ((size_t)m + CHOL_NB) * CHOL_NB * sizeof(float) + 16384;
}

// C (row-major lower block triangle, the part the Cholesky step reads) = M^T GM over `rows` rows of both.
// With the tile rows sharded over ranks every rank passes its own row range and the partial C are all-reduced.
// The transposed copy M^T (m x rows) at the start of the workspace has leading dimension pmd_gram_mtgm_ld(rows): a multiple of
// 64 floats.  (With ld = rows = 113 305 at BASELINE config 4 every row of the copy started off a 16-byte boundary and rocBLAS
// fell back to element-wise loads: 51 TFLOP/s for this product instead of 130.)
extern "C" long pmd_gram_mtgm_ld(int rows) { return pmd_round_up(rows, 64); }
extern "C" size_t pmd_gram_mtgm_workspace_bytes(int rows, int m) { return (size_t)m * pmd_gram_mtgm_ld(rows) * sizeof(float) + 4096; }

extern "C" int pmd_gram_mtgm(pmd_ctx* ctx, const float* M, int rows, int m, long ldm, const float* GM, long ldgm,
                             float* C, long ldc, void* ws, size_t ws_bytes) {
  CTX_CHECK(ctx);
  if (rows <= 0) return PMD_OK;
  pmd_arena ar(ws, ws_bytes);
  const long ldt = pmd_gram_mtgm_ld(rows);
  float* Mt = ar.take_n<float>((size_t)m * ldt);
  if (ar.overflow) return pmd_fail(ctx, PMD_ERR_WORKSPACE, "pmd_gram_mtgm", "workspace too small");
  // row blocks C[i0:i0+bs, 0:i0+bs] = Mt[i0:i0+bs, :] GM[:, 0:i0+bs]  (3/5 of the flops at 5 blocks)
  RUN(launch_transpose(ctx, M, ldm, rows, m, Mt, ldt));
  constexpr int MTGM_ROW_BLOCKS = 5;  // 2/3/4/5/6/8/12/16 blocks at m = 10^4: 70/64/57/52/59/58/60/67 ms
  const int bs = std::max(256, ((m + MTGM_ROW_BLOCKS - 1) / MTGM_ROW_BLOCKS + 255) / 256 * 256);
  // C is singular by construction on the R > frames route (its last pivot is the null direction, 3e-12 of the mean diagonal on
  // the headline fixture) and the Cholesky step needs every other pivot positive: this is the one product of the stage whose
  // error structure decides whether the route works at all.  Measured on that fixture (scripts/debug_headline.py): two fp16
  // pieces per operand (22-23 bits) fail the factorisation or pass it with wrong factors (s off by 0.57); THREE pieces hold an
  // fp32 number exactly, six of the nine piece products (down to 2^-22; the rest is 2^-33) are exact products accumulated in
  // fp32 - sgemm's own arithmetic - and then the length of the accumulation chain decides: chunks of 2048 / 3072 inner
  // indices pass with the figures of the fp32 path, chunks of 4096 and more fail.
  // PMD_F16X2_MTGM: 6 (default) = those six products as ONE matrix product per chunk of pmd_gemm_k_chunk(k) inner indices
  // (the "concatenated" form of gemm_f16x2.hip: C is revisited once per chunk, as on the fp32 path: 34 ms against 52 at
  // config 3, s 1.18e-4 / Vt 8.5e-4 / U R 1.05e-1 against the arbiter where sgemm gives 1.11e-4 / 1.2-1.5e-3 / 5.5-6.8e-2);
  // 0 = sgemm.  (Six separate products per chunk took 42 ms at config 3, but 870 against 690 ms at BASELINE config 4: C is
  // re-read and re-written six times per chunk.)
  // (not where the output is small and the inner dimension huge - the many-tile workloads: 10^3 x 10^3 outputs, k = 3 10^5 -
  // there one strided-batched split-K sgemm, pmd_gemm_rm, beats 150 chunks of tiny products)
  const long out_tiles = (long)((std::min(bs, m) + 127) / 128) * ((m + 127) / 128);
  if (ctx->routes.f16x2_mtgm == 6 && out_tiles >= 256 && pmd_f16x2_wanted(ctx, std::min(bs, m), m, rows)) {
    // the six piece products of three exact pieces per operand as ONE matrix product per accumulation chunk
    // (gemm_f16x2.hip, "concatenated" form): C is revisited once per chunk, as on the fp32 path, not six times
    const float* X[2] = {Mt, GM};
    const int xr[2] = {m, rows}, xc[2] = {rows, m};
    const long xl[2] = {ldt, ldgm};
    int ex[2] = {0, 0}, usable = 0;
    RUN(pmd_f16x2_exponents(ctx, 2, X, xr, xc, xl, ex, &usable));
    const int kc = pmd_gemm_k_chunk(ctx, rows);
    const long lda6 = 6L * pmd_round_up(kc, 8), ldb6 = pmd_round_up(m, 8);
    void* w = nullptr;
    if (usable) RUN(pmd_split_scratch(ctx, ((size_t)bs * lda6 + 6 * (size_t)kc * ldb6) * sizeof(_Float16) + 512, &w));
    const float alpha6 = ldexpf(1.f, ex[0] + ex[1]);
    if (usable && w && std::isfinite(alpha6) && alpha6 > 0.f) {
      _Float16* A6 = (_Float16*)w;
      _Float16* B6 = A6 + (size_t)bs * lda6;
      bool ok6 = true;
      for (int k0 = 0; k0 < rows && ok6; k0 += kc) {
        const int kk = std::min(kc, rows - k0);
        RUN(pmd_f16cat_b(ctx, GM + (long)k0 * ldgm, kk, m, ldgm, ex[1], B6, ldb6));
        for (int i0 = 0; i0 < m && ok6; i0 += bs) {
          const int nr = std::min(bs, m - i0);
          RUN(pmd_f16cat_a(ctx, Mt + (long)i0 * ldt + k0, nr, kk, ldt, ex[0], A6, lda6));
          int done = 0;
          RUN(pmd_f16_plain_matmul(ctx, nr, i0 + nr, 6 * kk, alpha6, A6, lda6, B6, ldb6, k0 ? 1.f : 0.f, C + (long)i0 * ldc, ldc, &done));
          if (!done) ok6 = false;
        }
        if (!ok6 && k0 > 0) return pmd_fail(ctx, PMD_ERR_BLAS, "pmd_gram_mtgm", "no hipBLASLt kernel for a later chunk");
      }
      if (ok6) return PMD_OK;
    }
  }
  for (int i0 = 0; i0 < m; i0 += bs) {
    const int nr = std::min(bs, m - i0);
    // the fp32 product: no piece route above produced this block, and pmd_gemm_rm's own fp16-piece product (two pieces in ONE
    // chain over all of `rows`, gemm_f16x2.hip) is the arithmetic that breaks this product (the many-tile workloads, where
    // the concatenated route is gated off, have row blocks above its size gate: 4x the fp32 error at 1000 x 309 827)
    const int keep = ctx->routes.gemm_split;
    ctx->routes.gemm_split = 0;
    const int rc = pmd_gemm_rm(ctx, 0, 0, nr, i0 + nr, rows, 1.f, Mt + (long)i0 * ldt, ldt, GM, ldgm, 0.f, C + (long)i0 * ldc, ldc);
    ctx->routes.gemm_split = keep;
    RUN(rc);
  }
  return PMD_OK;
}

// Small orders in double precision (the policy of pmd_syevd, sytrd.hip: global-stage problems up to order 512 are factorised
// in fp64 and rounded).  The Cholesky route amplifies the factorisation error by the condition number of C, which the
// reference's rank_prune and R > frames routes drive to 1e5 ... 1e7: in fp32 the signal singular values of such draws came
// out 27 % off where NumPy's (double-precision LAPACK on fp32 data) are 2 % off (seeded fuzz, options 104 / 42).
// Orders up to which the Cholesky step runs in double precision (rocSOLVER dpotrf + dtrtri on a widened copy, results
// rounded).  A constant: pmd_chol_inverse_workspace_bytes sizes the caller's buffer from it without a context.
constexpr int CHOL_F64_MAX = 512;

namespace {
__global__ void chol_widen_kernel(const float* __restrict__ src, long lds_, double* __restrict__ dst, long ldd, int n) {
  const int r = blockIdx.y;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) dst[(long)r * ldd + c] = (double)src[(long)r * lds_ + c];
}
// the factor lives in the row-major lower triangle; everything above the diagonal becomes zero
__global__ void chol_narrow_lower_kernel(const double* __restrict__ src, long lds_, float* __restrict__ dst, long ldd, int n) {
  const int r = blockIdx.y;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x)
    dst[(long)r * ldd + c] = (c <= r) ? (float)src[(long)r * lds_ + c] : 0.f;
}
// last pivot through its absolute value (abs_last_pivot of pmd_chol_inverse): memory row m - 1 holds y = U_11^{-T} c in its first
// m - 1 entries and C_mm in the last; U_mm = sqrt(|C_mm - y^T y|)
__global__ void chol_last_pivot_kernel(double* __restrict__ U, long ld, int m, int* __restrict__ info) {
  __shared__ double red[256];
  double* row = U + (long)(m - 1) * ld;
  double s = 0.0;
  for (int i = threadIdx.x; i < m - 1; i += 256) s += row[i] * row[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double p = row[m - 1] - red[0];
    if (!(fabs(p) > 0.0)) { if (*info == 0) *info = m; }
    else row[m - 1] = sqrt(fabs(p));
  }
}
}  // namespace

// In place: C = U_c^T U_c (row-major lower triangle read) -> Et = U_c^{-T} (row-major lower, rest zeroed).
extern "C" size_t pmd_chol_inverse_workspace_bytes(int m) {
  return ((size_t)m + CHOL_NB) * CHOL_NB * sizeof(float) + (m <= CHOL_F64_MAX ? (size_t)m * m * sizeof(double) + 64 : 0) + 8192;
}

extern "C" int pmd_chol_inverse(pmd_ctx* ctx, float* C, int m, long ldc, int abs_last_pivot, int* ok_host, void* ws,
                                size_t ws_bytes) {
  CTX_CHECK(ctx);
  pmd_arena ar(ws, ws_bytes);
  int* info = ar.take_n<int>(4);
  float* chol_tmp = ar.take_n<float>((size_t)m * CHOL_NB);
  float* chol_linv = ar.take_n<float>((size_t)CHOL_NB * CHOL_NB);
  const bool f64 = m <= CHOL_F64_MAX && m >= 1 && !ctx->routes.cholesky_rocsolver;
  double* Cd = f64 ? ar.take_n<double>((size_t)m * m) : nullptr;
  if (ar.overflow) return pmd_fail(ctx, PMD_ERR_WORKSPACE, "pmd_chol_inverse", "workspace too small");   // (*ok_host untouched)
  *ok_host = 0;
  int hinfo = 0;
  if (f64) {
    pmd_prof_scope prof__(ctx, "cholesky_f64");
    PMD_HIP(ctx, hipMemsetAsync(info, 0, 2 * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(chol_widen_kernel, dim3((m + 255) / 256, m), dim3(256), 0, ctx->stream, C, ldc, Cd, (long)m, m);
    PMD_LAUNCH_CHECK(ctx, "chol_widen_kernel");
    // the row-major lower triangle is the column-major upper one: C = U^T U
    const int mf = abs_last_pivot ? m - 1 : m;
    if (mf > 0) PMD_BLAS(ctx, rocsolver_dpotrf(ctx->blas, rocblas_fill_upper, mf, Cd, m, info));
    if (abs_last_pivot) {
      if (m > 1)
        PMD_BLAS(ctx, rocblas_dtrsv(ctx->blas, rocblas_fill_upper, rocblas_operation_transpose, rocblas_diagonal_non_unit, m - 1, Cd, m,
                                    Cd + (long)(m - 1) * m, 1));
      hipLaunchKernelGGL(chol_last_pivot_kernel, dim3(1), dim3(256), 0, ctx->stream, Cd, (long)m, m, info + 1);
      PMD_LAUNCH_CHECK(ctx, "chol_last_pivot_kernel");
    }
    int h2[2] = {0, 0};
    PMD_HIP(ctx, hipMemcpyAsync(h2, info, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h2[0] != 0 || h2[1] != 0) return PMD_OK;   // not positive definite: ok_host stays 0, C is untouched
    PMD_BLAS(ctx, rocsolver_dtrtri(ctx->blas, rocblas_fill_upper, rocblas_diagonal_non_unit, m, Cd, m, info));
    PMD_HIP(ctx, hipMemcpyAsync(h2, info, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    hipLaunchKernelGGL(chol_narrow_lower_kernel, dim3((m + 255) / 256, m), dim3(256), 0, ctx->stream, Cd, (long)m, C, ldc, m);
    PMD_LAUNCH_CHECK(ctx, "chol_narrow_lower_kernel");
    PMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h2[0] != 0) return pmd_fail(ctx, PMD_ERR_BLAS, "rocsolver_dtrtri", "singular factor");
    *ok_host = 1;
    return PMD_OK;
  }
  if (ctx->routes.cholesky_rocsolver && !abs_last_pivot) {
    pmd_prof_scope prof__(ctx, "rocsolver_spotrf");
    PMD_BLAS(ctx, rocsolver_spotrf(ctx->blas, rocblas_fill_upper, m, C, (rocblas_int)ldc, info));
  } else {
    RUN(chol_lower_rm(ctx, m, C, ldc, info, chol_tmp, chol_linv, abs_last_pivot));
  }
  PMD_HIP(ctx, hipMemcpyAsync(&hinfo, info, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  PMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (hinfo != 0) return PMD_OK;  // not positive definite: ok_host stays 0
  {
    pmd_prof_scope prof__(ctx, "rocsolver_strtri");
    PMD_BLAS(ctx, rocsolver_strtri(ctx->blas, rocblas_fill_upper, rocblas_diagonal_non_unit, m, C, (rocblas_int)ldc, info));
  }
  PMD_HIP(ctx, hipMemcpyAsync(&hinfo, info, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  // column-major upper U^{-1} == row-major lower U^{-T} = Et; clear the other triangle (old C entries)
  hipLaunchKernelGGL(tril_mask_kernel, dim3(8, m), dim3(256), 0, ctx->stream, C, ldc, m);
  PMD_LAUNCH_CHECK(ctx, "tril_mask_kernel");
  PMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (hinfo != 0) return PMD_OK;
  *ok_host = 1;
  return PMD_OK;
}

extern "C" int pmd_orthogonalize_chol(pmd_ctx* ctx, const float* M, int Rc, int m, long ldm, const float* GM, long ldgm,
                                      float* Et_out, long lde, int* ok_host, void* ws, size_t ws_bytes) {
  CTX_CHECK(ctx);
  // both halves carve the same workspace: refuse one that the second half would refuse before the first has launched anything
  if (!ws || ws_bytes < std::max(pmd_gram_mtgm_workspace_bytes(Rc, m), pmd_chol_inverse_workspace_bytes(m)))
    return pmd_fail(ctx, PMD_ERR_WORKSPACE, "pmd_orthogonalize_chol", "workspace too small");
  RUN(pmd_gram_mtgm(ctx, M, Rc, m, ldm, GM, ldgm, Et_out, lde, ws, ws_bytes));
  return pmd_chol_inverse(ctx, Et_out, m, lde, 0, ok_host, ws, ws_bytes);
}
