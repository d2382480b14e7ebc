// Global recombination: the GEMM entry, the orthogonalising mixing matrix P, V projection helpers and the projected SVD
// (decomposition.py:912-1137, pmd_loader.py:316-346, :392-414).  G = U^T U itself is in gram.hip, the Cholesky form of the
// orthogonalisation in chol.hip.
// Dense fp32 GEMMs go to rocBLAS and the dense symmetric eigenproblem to rocSOLVER (ssyevd);
// everything else is hand-written.  Matrices are row-major; the rocBLAS calls use the usual
// operand swap (C^T = B^T A^T).
#include "pmd_internal.h"
#include <algorithm>
#include <cmath>
#include <vector>

// row-major C(m x n) = alpha * op(A) * op(B) + beta * C
// ---------------------------------------------------------------- long inner dimension ------
// A product with few output tiles and a very long inner dimension (M^T G M and M^T Z when R = 3e5 tile components meet
// 1e3 frames: 1000 x 1000 outputs, k = 3e5) leaves most CUs idle in rocBLAS' sgemm (measured 20 TFLOP/s on the many-tile
// workloads).  The inner dimension is cut into S slices that run as ONE strided-batched sgemm (S x the workgroups) into
// S partial outputs, which a second kernel sums in a fixed order (reproducible).
__global__ void sum_partials_kernel(const float* __restrict__ part, long mn, int n, int S, float beta, float* __restrict__ C, long ldc) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < mn; i += (long)gridDim.x * blockDim.x) {
    const long r = i / n;
    const int c = (int)(i - r * n);
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += part[(long)s * mn + i];
    float* o = C + r * ldc + c;
    *o = (beta == 0.f) ? acc : acc + beta * *o;
  }
}

// Length of one fp32 accumulation chain in the library's GEMM-shaped products (PMD_GEMM_KCHUNK overrides; 0 = whole k):
// 1024 up to k = 16384, 2048 beyond (the output is re-read once per chunk: 12 % / 6 % of the product's time).
int pmd_gemm_k_chunk(const pmd_ctx* ctx, int k) {
  const int forced = ctx->routes.gemm_kchunk;
  if (forced == 0) return k;
  if (forced > 0) return forced;
  if (k <= 3072) return k;
  return k <= 16384 ? 1024 : 2048;
}

static bool pmd_is_host_pointer(const void* p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return attr.type == hipMemoryTypeHost;
}

static int gemm_rm_splitk(pmd_ctx* ctx, int transA, int transB, int m, int n, int k, int S, float alpha, const float* A, long lda,
                          const float* B, long ldb, float beta, float* C, long ldc) {
  pmd_prof_scope prof__(ctx, "rocblas_sgemm_splitk");
  const int kc = (k + S - 1) / S;
  const int full = k / kc, rem = k - full * kc;   // `full` slices of kc, one more of `rem`
  const int slices = full + (rem ? 1 : 0);
  const long mn = (long)m * n;
  const size_t need = (size_t)slices * mn * sizeof(float) + 4096;
  void* scratch = nullptr;
  RUN(pmd_split_scratch(ctx, need, &scratch));
  if (!scratch) return pmd_fail(ctx, PMD_ERR_HIP, "gemm_rm_splitk", "out of device memory for the partial sums");
  float* part = (float*)scratch;
  const float zero = 0.f;
  const rocblas_operation opA = transA ? rocblas_operation_transpose : rocblas_operation_none;
  const rocblas_operation opB = transB ? rocblas_operation_transpose : rocblas_operation_none;
  // slice s covers inner indices [s kc, (s + 1) kc): A advances by kc columns (or rows when transposed), B by kc rows (columns)
  const long strideA = transA ? (long)kc * lda : kc, strideB = transB ? kc : (long)kc * ldb;
  PMD_BLAS(ctx, rocblas_sgemm_strided_batched(ctx->blas, opB, opA, n, m, kc, &alpha, B, (rocblas_int)ldb, strideB, A, (rocblas_int)lda,
                                              strideA, &zero, part, n, mn, full));
  if (rem)
    PMD_BLAS(ctx, rocblas_sgemm(ctx->blas, opB, opA, n, m, rem, &alpha, B + (long)full * strideB, (rocblas_int)ldb,
                                A + (long)full * strideA, (rocblas_int)lda, &zero, part + (long)full * mn, n));
  hipLaunchKernelGGL(sum_partials_kernel, dim3((unsigned)std::min<long>((mn + 255) / 256, 4096)), dim3(256), 0, ctx->stream, part, mn, n,
                     slices, beta, C, ldc);
  PMD_LAUNCH_CHECK(ctx, "sum_partials_kernel");
  return PMD_OK;
}

int pmd_gemm_rm(pmd_ctx* ctx, int transA, int transB, int m, int n, int k, float alpha, const float* A, long lda,
                const float* B, long ldb, float beta, float* C, long ldc) {
  if (m <= 0 || n <= 0) return PMD_OK;
  if (k > 0 && pmd_f16x2_wanted(ctx, m, n, k) && !pmd_is_host_pointer(C)) {
    // large products: three fp16-piece products on the fp16 matrix cores, error below the fp32 path's (gemm_f16x2.hip);
    // done = 0 (Inf / NaN / all-zero operands, no kernel for the shape): C is untouched and the fp32 path below runs
    int done = 0;
    RUN(pmd_gemm_f16x2(ctx, transA, transB, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, &done));
    if (done) return PMD_OK;
  }
  {
    // fewer than one 128 x 128 output tile per CU and an inner dimension that leaves >= 4096 per slice
    // (PMD_GEMM_SPLITK=0 switches the path off, A/B runs)
    const long tiles = (long)((m + 127) / 128) * ((n + 127) / 128);
    if (ctx->routes.gemm_splitk && tiles < 256 && k >= 16384) {
      int S = (int)std::min<long>(std::min<long>(64, k / 4096), (512 + tiles - 1) / tiles);
      if (S >= 2) return gemm_rm_splitk(ctx, transA, transB, m, n, k, S, alpha, A, lda, B, ldb, beta, C, ldc);
    }
  }
  pmd_prof_scope prof__(ctx, "rocblas_sgemm");
  const int kc = pmd_gemm_k_chunk(ctx, k);
  if (kc < k && !pmd_is_host_pointer(C)) {
    // Long inner dimension: rocBLAS carries ONE fp32 accumulation chain over all of k (measured on MI355X, scripts/
    // gemm_bias_probe.py: entry errors of 4.9e-6 of the diagonal at k = 10^4, against 3.8e-7 when the chain is cut every
    // 1024 terms - what a CPU BLAS does through its k blocking, and what the NumPy oracle therefore sees).  On the Gram
    // matrix of a 2000 x 10^4 trace matrix those entry errors add up to 4e-5 on the leading singular values and 6e-4 on
    // right singular vectors with 2 % gaps.  Chunks of kc terms accumulated into C (one rounding per chunk).
    const rocblas_operation opA = transA ? rocblas_operation_transpose : rocblas_operation_none;
    const rocblas_operation opB = transB ? rocblas_operation_transpose : rocblas_operation_none;
    const float one = 1.f;
    for (int k0 = 0; k0 < k; k0 += kc) {
      const int kk = std::min(kc, k - k0);
      const float* a = A + (transA ? (long)k0 * lda : (long)k0);
      const float* b = B + (transB ? (long)k0 : (long)k0 * ldb);
      PMD_BLAS(ctx, rocblas_sgemm(ctx->blas, opB, opA, n, m, kk, &alpha, b, (rocblas_int)ldb, a, (rocblas_int)lda, k0 == 0 ? &beta : &one, C,
                                  (rocblas_int)ldc));
    }
    return PMD_OK;
  }
  PMD_BLAS(ctx, rocblas_sgemm(ctx->blas, transB ? rocblas_operation_transpose : rocblas_operation_none,
                              transA ? rocblas_operation_transpose : rocblas_operation_none, n, m, k, &alpha, B,
                              (rocblas_int)ldb, A, (rocblas_int)lda, &beta, C, (rocblas_int)ldc));
  return PMD_OK;
}

extern "C" int pmd_gemm(pmd_ctx* ctx, int transA, int transB, int m, int n, int k, float alpha, const float* A, long lda, const float* B,
                        long ldb, float beta, float* C, long ldc) {
  CTX_CHECK(ctx);
  return pmd_gemm_rm(ctx, transA, transB, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc);
}

// ---------------------------------------------------------------- helpers for eigen output -
// dst[c][x] = src[perm[c]][x] * scale[c]   (row gather of the eigenvector matrix)
__global__ void gather_rows_scale_kernel(const float* __restrict__ src, long lds_, const int* __restrict__ perm,
                                         const float* __restrict__ scale, int ncols, float* __restrict__ dst, long ldd) {
  const int c = blockIdx.y;
  const float s = scale[c];
  const long r = perm[c];
  for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < ncols; x += gridDim.x * blockDim.x)
    dst[(long)c * ldd + x] = src[r * lds_ + x] * s;
}

__global__ void transpose_kernel(const float* __restrict__ src, long lds_, int rows, int cols, float* __restrict__ dst,
                                 long ldd) {
  __shared__ float t[32][33];
  const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8)
    if (y0 + r < rows && x0 + tx < cols) t[r][tx] = src[(long)(y0 + r) * lds_ + x0 + tx];
  __syncthreads();
  for (int r = ty; r < 32; r += 8)
    if (x0 + r < cols && y0 + tx < rows) dst[(long)(x0 + r) * ldd + y0 + tx] = t[tx][r];
}

__global__ void scale_rows2_kernel(float* __restrict__ x, long ld, int ncols, const float* __restrict__ scale) {
  const float s = scale[blockIdx.y];
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncols; c += gridDim.x * blockDim.x) x[(long)blockIdx.y * ld + c] *= s;
}

__global__ void scale_cols_kernel(float* __restrict__ x, long ld, int ncols, const float* __restrict__ scale) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncols; c += gridDim.x * blockDim.x) x[(long)blockIdx.y * ld + c] *= scale[c];
}

int launch_gather_rows(pmd_ctx* ctx, const float* src, long lds_, const int* perm, const float* scale, int nrows,
                       int ncols, float* dst, long ldd) {
  for (int r0 = 0; r0 < nrows; r0 += 32768) {
    const int rn = (nrows - r0 < 32768) ? nrows - r0 : 32768;
    hipLaunchKernelGGL(gather_rows_scale_kernel, dim3(8, rn), dim3(256), 0, ctx->stream, src, lds_, perm + r0,
                       scale + r0, ncols, dst + (long)r0 * ldd, ldd);
    PMD_LAUNCH_CHECK(ctx, "gather_rows_scale_kernel");
  }
  return PMD_OK;
}

int launch_transpose(pmd_ctx* ctx, const float* src, long lds_, int rows, int cols, float* dst, long ldd) {
  hipLaunchKernelGGL(transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0, ctx->stream, src, lds_,
                     rows, cols, dst, ldd);
  PMD_LAUNCH_CHECK(ctx, "transpose_kernel");
  return PMD_OK;
}

// ---------------------------------------------------------------- eigen-solve epilogue -----
// Device buffers of an eigen-solve of order n, taken from a workspace in this order: w, work (n floats each), one or two
// upload vectors f0, f1 (n floats), perm (n ints), info.
struct eig_bufs {
  float *w, *work, *f0, *f1;
  int *perm, *info;
  eig_bufs(pmd_arena& ar, int n, bool two)
      : w(ar.take_n<float>(n)), work(ar.take_n<float>(n)), f0(ar.take_n<float>(n)), f1(two ? ar.take_n<float>(n) : nullptr),
        perm(ar.take_n<int>(n)), info(ar.take_n<int>(4)) {}
};

// Host side of the same: the eigenvalues as read back, their order, and the vectors uploaded from them.  The uploads are
// asynchronous: the caller keeps this alive until its next hipStreamSynchronize.
struct eig_host {
  std::vector<float> w, scale, s, sgn, inv;
  std::vector<int> idx, perm;
};

// pmd_syevd of A (n x n, eigenvectors come back as its rows); h.w = the eigenvalues, h.idx = their order by |lambda|
// descending (stable: jnp.linalg.svd(hermitian=True)).  Host sync: the eigenvalues come back.
static int eig_solve_sorted(pmd_ctx* ctx, int n, float* A, long lda, const eig_bufs& d, eig_host& h) {
  RUN(pmd_syevd(ctx, n, A, lda, d.w, d.work, d.info));
  h.w.resize(n);
  int hinfo = 0;
  PMD_HIP(ctx, hipMemcpyAsync(h.w.data(), d.w, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  PMD_HIP(ctx, hipMemcpyAsync(&hinfo, d.info, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  PMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (hinfo != 0) return pmd_fail(ctx, PMD_ERR_BLAS, "rocsolver_ssyevd", "did not converge");
  h.idx.resize(n);
  for (int i = 0; i < n; ++i) h.idx[i] = i;
  std::stable_sort(h.idx.begin(), h.idx.end(), [&](int a, int b) { return std::fabs(h.w[a]) > std::fabs(h.w[b]); });
  return PMD_OK;
}

// Orthogonaliser: rows of Et (ld lde) = the kept eigenvectors of C (m x m, overwritten) / sqrt|lambda| with the sign of
// lambda, *rprime_out of them.
// jnp.linalg.svd(hermitian=True) returns |lambda| and u = v sign(lambda): `eig_vals > 0` (decomposition.py:988)
// keeps every direction whose eigenvalue is not exactly zero.  null_cutoff >= 0 (pmd_ctx_set_null_cutoff):
// only lambda > cutoff * lambda_max.
static int eig_orthogonaliser(pmd_ctx* ctx, int m, float* C, long ldc, const eig_bufs& d, eig_host& h, float* Et, long lde,
                              int* rprime_out) {
  RUN(eig_solve_sorted(ctx, m, C, ldc, d, h));
  const float lmax = m > 0 ? std::fabs(h.w[h.idx[0]]) : 0.f;
  for (int i = 0; i < m; ++i) {
    const float lam = h.w[h.idx[i]];
    const bool keep = ctx->null_cutoff < 0.f ? (lam != 0.f && lam == lam) : (lam > ctx->null_cutoff * lmax);
    if (keep) {
      h.perm.push_back(h.idx[i]);
      h.scale.push_back((lam < 0.f ? -1.0f : 1.0f) / std::sqrt(std::fabs(lam)));
    }
  }
  const int rp = (int)h.perm.size();
  *rprime_out = rp;
  if (rp == 0) return PMD_OK;
  PMD_HIP(ctx, hipMemcpyAsync(d.perm, h.perm.data(), (size_t)rp * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  PMD_HIP(ctx, hipMemcpyAsync(d.f0, h.scale.data(), (size_t)rp * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  return launch_gather_rows(ctx, C, ldc, d.perm, d.f0, rp, m, Et, lde);
}

// Singular values from a Gram matrix C (n x n, overwritten), all directions: s_out[c] = sqrt|lambda_c| (device),
// Wt[c][:] = sign_c * eigenvector c (n x n), d.f1[c] = 1 / s_c (1 where s_c = 0).
static int eig_singular(pmd_ctx* ctx, int n, float* C, long ldc, const eig_bufs& d, eig_host& h, float* s_out, float* Wt) {
  RUN(eig_solve_sorted(ctx, n, C, ldc, d, h));
  h.s.resize(n), h.sgn.resize(n), h.inv.resize(n);
  for (int i = 0; i < n; ++i) {
    const float lam = h.w[h.idx[i]];
    h.s[i] = std::sqrt(std::fabs(lam));
    h.sgn[i] = (lam < 0.f) ? -1.f : 1.f;
    h.inv[i] = (h.s[i] == 0.f) ? 1.f : 1.f / h.s[i];
  }
  PMD_HIP(ctx, hipMemcpyAsync(d.perm, h.idx.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  PMD_HIP(ctx, hipMemcpyAsync(d.f0, h.sgn.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  PMD_HIP(ctx, hipMemcpyAsync(d.f1, h.inv.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  PMD_HIP(ctx, hipMemcpyAsync(s_out, h.s.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  return launch_gather_rows(ctx, C, ldc, d.perm, d.f0, n, n, Wt, n);
}

// ---------------------------------------------------------------- A15 ----------------------
// compute_lowrank_factorized_svd(only_left=True), decomposition.py:974-999.
// G: R x R (overwritten).  M: R x m right matrix (row-major, ldm) or NULL for the identity
// (reference: right_mat = v if R > v.shape[1] else eye(R)).  P_out: R x R' (ldp >= m).
// Host sync: the eigenvalues come back to count R' (reference: good_components = eig_vals > 0).
extern "C" size_t pmd_orthogonalize_workspace_bytes(int R, int m, int has_m) {
  size_t b = 0;
  b += (size_t)m * sizeof(float) * 4 + (size_t)m * sizeof(int) + 4096;  // w, work, scale, perm, info
  if (has_m) b += (size_t)R * m * sizeof(float) + (size_t)m * m * sizeof(float);  // GM, C
  b += (size_t)m * m * sizeof(float);                                             // Et
  return b + 8192;   // slack by design: the 4096 above already covers the at most 8 x 255 bytes of arena padding
}

extern "C" int pmd_orthogonalize(pmd_ctx* ctx, float* G, int R, const float* M, int m, long ldm, float* P_out, long ldp,
                                 int* rprime_out, void* ws, size_t ws_bytes) {
  CTX_CHECK(ctx);
  pmd_arena ar(ws, ws_bytes);
  const eig_bufs eb(ar, m, false);
  float* C = nullptr;
  float* GM = nullptr;
  if (M) {
    GM = ar.take_n<float>((size_t)R * m);
    C = ar.take_n<float>((size_t)m * m);
  } else {
    if (m != R) return pmd_fail(ctx, PMD_ERR_ARG, "pmd_orthogonalize", "identity right matrix needs m == R");
    C = G;
  }
  float* Et = ar.take_n<float>((size_t)m * m);
  if (ar.overflow) return pmd_fail(ctx, PMD_ERR_WORKSPACE, "pmd_orthogonalize", "workspace too small");
  long ldc = M ? m : R;
  if (M) {
    RUN(pmd_gemm_rm(ctx, 0, 0, R, m, R, 1.f, G, R, M, ldm, 0.f, GM, m));
    RUN(pmd_gemm_rm(ctx, 1, 0, m, m, R, 1.f, M, ldm, GM, m, 0.f, C, m));
  }
  eig_host eh;
  RUN(eig_orthogonaliser(ctx, m, C, ldc, eb, eh, Et, m, rprime_out));
  const int rp = *rprime_out;
  if (rp == 0) return PMD_OK;
  if (M) RUN(pmd_gemm_rm(ctx, 0, 1, R, rp, m, 1.f, M, ldm, Et, m, 0.f, P_out, ldp));
  else RUN(launch_transpose(ctx, Et, m, rp, m, P_out, ldp));
  PMD_HIP(ctx, hipStreamSynchronize(ctx->stream));  // eh's vectors are host temporaries
  return PMD_OK;
}

// ---------------------------------------------------------------- A17 ----------------------
// projected_svd (decomposition.py:1042-1060) with fewer_rows (:1089-1099) / fewer_columns
// (:1128-1137).  V: n1 x n2 (row-major, preserved).
// Outputs: R_out (rows_p x nk), s_out (nk), Vt_out (nk x n2), nk = min(n1, n2).

// Gram matrix of V over its k columns (rows: V V^T, V n x k) or its k rows (V^T V, V k x n): only the row-major upper
// triangle (= column-major lower) of C (n x n), the one pmd_syevd reads.
// (inner dimension in chunks: one fp32 accumulation chain per chunk, see pmd_gemm_rm)
static int psvd_gram(pmd_ctx* ctx, bool rows, const float* V, int n, int k, long ldv, float* C, long ldc) {
  pmd_prof_scope prof__(ctx, "rocblas_ssyrk");
  const float one = 1.f, zero = 0.f;
  const int kc = pmd_gemm_k_chunk(ctx, k);
  if (k <= 0) { PMD_HIP(ctx, hipMemsetAsync(C, 0, (size_t)n * ldc * sizeof(float), ctx->stream)); return PMD_OK; }
  for (int k0 = 0; k0 < k; k0 += kc) {
    const int kk = std::min(kc, k - k0);
    PMD_BLAS(ctx, rocblas_ssyrk(ctx->blas, rocblas_fill_lower, rows ? rocblas_operation_transpose : rocblas_operation_none, n, kk, &one,
                                rows ? V + k0 : V + (long)k0 * ldv, (rocblas_int)ldv, k0 == 0 ? &zero : &one, C, (rocblas_int)ldc));
  }
  return PMD_OK;
}

// n1 <= n2 from the Gram matrix C = V V^T (n1 x n1, overwritten; possibly summed over column parts of which V, n1 x n2,
// is one): s_out, Wt (row c = left vector c, sign included) and Vt_out = (W^T V) / s.
static int psvd_rows_core(pmd_ctx* ctx, float* C, long ldc, int n1, const float* V, int n2, long ldv, const eig_bufs& d, eig_host& h,
                          float* Wt, float* s_out, float* Vt_out, long ldvt) {
  RUN(eig_singular(ctx, n1, C, ldc, d, h, s_out, Wt));
  if (n2 > 0) {
    RUN(pmd_gemm_rm(ctx, 0, 0, n1, n2, n1, 1.f, Wt, n1, V, ldv, 0.f, Vt_out, ldvt));
    hipLaunchKernelGGL(scale_rows2_kernel, dim3(8, n1), dim3(256), 0, ctx->stream, Vt_out, ldvt, n2, d.f1);
    PMD_LAUNCH_CHECK(ctx, "scale_rows2_kernel");
  }
  return PMD_OK;
}

extern "C" size_t pmd_projected_svd_workspace_bytes(int rows_p, int n1, int n2) {
  const size_t nk = (size_t)std::min(n1, n2);
  size_t b = (nk + 4) * nk * sizeof(float) * 2 + nk * (sizeof(float) * 5 + sizeof(int)) + 8192;
  if (n1 > n2) b += (size_t)n1 * n2 * sizeof(float);
  return b + 8192;
}

extern "C" int pmd_projected_svd(pmd_ctx* ctx, const float* P, int rows_p, long ldp, const float* V, int n1, int n2,
                                 long ldv, float* R_out, long ldr, float* s_out, float* Vt_out, long ldvt, void* ws,
                                 size_t ws_bytes) {
  CTX_CHECK(ctx);
  const int nk = std::min(n1, n2);
  pmd_arena ar(ws, ws_bytes);
  const long ldc = pmd_round_up(nk, 4);  // the library's own tridiagonalisation wants 16-byte aligned rows
  float* C = ar.take_n<float>((size_t)ldc * nk);
  float* Wt = ar.take_n<float>((size_t)nk * nk);
  const eig_bufs eb(ar, nk, true);
  float* left = (n1 > n2) ? ar.take_n<float>((size_t)n1 * n2) : nullptr;
  if (ar.overflow) return pmd_fail(ctx, PMD_ERR_WORKSPACE, "pmd_projected_svd", "workspace too small");
  eig_host eh;
  if (n1 <= n2) {
    // Vt = (W^T V) / s ; R = P W
    RUN(psvd_gram(ctx, true, V, n1, n2, ldv, C, ldc));
    RUN(psvd_rows_core(ctx, C, ldc, n1, V, n2, ldv, eb, eh, Wt, s_out, Vt_out, ldvt));
    if (P) RUN(pmd_gemm_rm(ctx, 0, 1, rows_p, nk, n1, 1.f, P, ldp, Wt, nk, 0.f, R_out, ldr));
    else RUN(launch_transpose(ctx, Wt, nk, nk, n1, R_out, ldr));  // no projection: R_out = W (n1 x nk)
  } else {
    // right_t = W; left = V (W / s); R = P left; Vt = W^T
    RUN(psvd_gram(ctx, false, V, n2, n1, ldv, C, ldc));
    RUN(eig_singular(ctx, nk, C, ldc, eb, eh, s_out, Wt));
    RUN(pmd_gemm_rm(ctx, 0, 1, n1, nk, n2, 1.f, V, ldv, Wt, nk, 0.f, left, nk));
    hipLaunchKernelGGL(scale_cols_kernel, dim3(8, n1), dim3(256), 0, ctx->stream, left, (long)nk, nk, eb.f1);
    PMD_LAUNCH_CHECK(ctx, "scale_cols_kernel");
    RUN(pmd_gemm_rm(ctx, 0, 0, rows_p, nk, n1, 1.f, P, ldp, left, nk, 0.f, R_out, ldr));
    PMD_HIP(ctx, hipMemcpy2DAsync(Vt_out, ldvt * sizeof(float), Wt, (size_t)nk * sizeof(float), (size_t)nk * sizeof(float), nk, hipMemcpyDeviceToDevice, ctx->stream));
  }
  PMD_HIP(ctx, hipStreamSynchronize(ctx->stream));   // eh's vectors are host temporaries
  return PMD_OK;
}

// ---------------------------------------------------------------- A17 split by frame columns ------------------
// Multi-GPU form of the factored projected SVD (the frames x frames products of the last stage sharded by frame columns):
//   pmd_psvd_vp_gram : Vp_r = Et W1[:, c0:c1) for this rank's frame columns, C_r = Vp_r Vp_r^T (row-major upper triangle)
//   [the caller sums C_r over the ranks]
//   pmd_psvd_finish  : eigendecomposition of the summed C (replicated), s, W, and this rank's columns of Vt = W^T Vp / s
// One rank with all columns reproduces pmd_projected_svd_factored (the same functions in the same order).

// Vp (rp x nc) = Et (rp x m) W1 (m x nc).  Cholesky route: Et is lower triangular (zeros above the diagonal), strmm does
// half the work in fp32; where the full product runs from fp16 pieces (gemm_f16x2.hip) that is faster still (6 against
// 10 ms at order 10^4)
static int psvd_vp(pmd_ctx* ctx, const float* Et, int rp, int m, long lde, const float* W1, int nc, long ldw, int et_lower, float* Vp,
                   long ldv) {
  if (et_lower && rp == m && !pmd_f16x2_wanted(ctx, rp, nc, m)) {
    // row-major Vp = Et W1  <=>  column-major Vp^T = W1^T Et^T with Et^T upper on the right
    pmd_prof_scope prof__(ctx, "rocblas_strmm");
    const float one = 1.f;
    PMD_BLAS(ctx, rocblas_strmm(ctx->blas, rocblas_side_right, rocblas_fill_upper, rocblas_operation_none, rocblas_diagonal_non_unit, nc, m,
                                &one, Et, (rocblas_int)lde, W1, (rocblas_int)ldw, Vp, (rocblas_int)ldv));
    return PMD_OK;
  }
  return pmd_gemm_rm(ctx, 0, 0, rp, nc, m, 1.f, Et, lde, W1, ldw, 0.f, Vp, ldv);
}

extern "C" int pmd_psvd_vp_gram(pmd_ctx* ctx, const float* Et, int rp, int m, long lde, const float* W1, int nc,
                                long ldw, int et_lower, float* Vp, long ldv, float* C, long ldc) {
  CTX_CHECK(ctx);
  if (rp < 1 || m < rp || nc < 0 || ldc < rp) return pmd_fail(ctx, PMD_ERR_ARG, "pmd_psvd_vp_gram", "bad shape");
  if (nc > 0) RUN(psvd_vp(ctx, Et, rp, m, lde, W1, nc, ldw, et_lower, Vp, ldv));
  return psvd_gram(ctx, true, Vp, rp, nc, ldv, C, ldc);
}

extern "C" size_t pmd_psvd_finish_workspace_bytes(int rp) {
  return (size_t)rp * rp * sizeof(float) + (size_t)rp * (sizeof(float) * 5 + sizeof(int)) + 16384;
}

// C: summed Gram matrix (rp x rp, ld ldc >= round_up(rp, 4); overwritten), Vp: this rank's columns (rp x nc).
// Outputs: W_out (rp x rp, row c' = component c' of the left vectors, i.e. W[c'][c]), s_out (rp), Vt_out (rp x nc).
extern "C" int pmd_psvd_finish(pmd_ctx* ctx, float* C, long ldc, int rp, const float* Vp, int nc, long ldv,
                               float* W_out, long ldw, float* s_out, float* Vt_out, long ldvt, void* ws,
                               size_t ws_bytes) {
  CTX_CHECK(ctx);
  if (rp < 1 || nc < 0 || ldc < rp) return pmd_fail(ctx, PMD_ERR_ARG, "pmd_psvd_finish", "bad shape");
  pmd_arena ar(ws, ws_bytes);
  float* Wt = ar.take_n<float>((size_t)rp * rp);
  const eig_bufs eb(ar, rp, true);
  if (ar.overflow) return pmd_fail(ctx, PMD_ERR_WORKSPACE, "pmd_psvd_finish", "workspace too small");
  eig_host eh;
  RUN(psvd_rows_core(ctx, C, ldc, rp, Vp, nc, ldv, eb, eh, Wt, s_out, Vt_out, ldvt));
  RUN(launch_transpose(ctx, Wt, rp, rp, rp, W_out, ldw));
  PMD_HIP(ctx, hipStreamSynchronize(ctx->stream));   // eh's vectors are host temporaries
  return PMD_OK;
}

// ---------------------------------------------------------------- background projection ----
// out[k][t] = sum_c basis[c][k] * xs[c][t]  (pmd_loader.py:386, and the K background rows of
// U^T X in :411).  xs must have round_up(D, 1024) rows allocated (rows >= D zero).
#define BGP_BLK 1024

__global__ void block_basis_kernel(const float* __restrict__ basis, long D, int K, float* __restrict__ At, int kstride) {
  // At[blk][k][q] = basis[blk*BGP_BLK + q][k]   (K <= 64 columns of a basis with kstride columns per pixel)
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long blk = c / BGP_BLK;
  const int q = (int)(c - blk * BGP_BLK);
  for (int k = 0; k < PMD_RPAD; ++k) At[blk * PMD_RPAD * BGP_BLK + (long)k * BGP_BLK + q] = (c < D && k < K) ? basis[c * kstride + k] : 0.f;
}

extern "C" size_t pmd_bg_project_workspace_bytes(long D, int T) {
  const size_t nblk = (size_t)((D + BGP_BLK - 1) / BGP_BLK);
  return nblk * 64 * BGP_BLK * sizeof(float) + nblk * 64 * (size_t)pmd_time_ld(T) * sizeof(float) + 8192;
}

extern "C" int pmd_bg_project(pmd_ctx* ctx, const float* xs, long D, int T, long ld, const float* basis, int K,
                              float* out, long ldo, void* ws, size_t ws_bytes) {
  CTX_CHECK(ctx);
  if (K < 1) return pmd_fail(ctx, PMD_ERR_ARG, "pmd_bg_project", "background rank must be >= 1");
  const int nblk = (int)((D + BGP_BLK - 1) / BGP_BLK);
  const long ldt = pmd_time_ld(T);
  pmd_arena ar(ws, ws_bytes);
  float* At = ar.take_n<float>((size_t)nblk * 64 * BGP_BLK);
  float* part = ar.take_n<float>((size_t)nblk * 64 * ldt);
  if (ar.overflow) return pmd_fail(ctx, PMD_ERR_WORKSPACE, "pmd_bg_project", "workspace too small");
  // 64 basis columns per pass over the movie (ranks above 64: several passes)
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int kc = (K - k0 < 64) ? K - k0 : 64;
    hipLaunchKernelGGL(block_basis_kernel, dim3(nblk * (BGP_BLK / 256)), dim3(256), 0, ctx->stream, basis + k0, D, kc, At, K);
    PMD_LAUNCH_CHECK(ctx, "block_basis_kernel");
    // (<= 16 columns - the default rank is 15 - run on one row tile: a quarter of the MFMA work)
    RUN(pmd_launch_tile_atx(ctx, xs, ld, nullptr, 0, BGP_BLK, BGP_BLK, At, 64L * BGP_BLK, BGP_BLK, part, 64L * ldt, ldt, nblk, T, 8,
                            {"tile_atx", kc}));
    // sum the block partials row by row into out[k][0:T]
    for (int k = 0; k < kc; ++k)
      RUN(pmd_launch_reduce_slices(ctx, part + (long)k * ldt, 0, 64L * ldt, nblk, T, out + (long)(k0 + k) * ldo, 0, 1));
  }
  return PMD_OK;
}

// =============================================================================================
// Factored form of A15 + A16 + A17 for R > frames (P = M E^T is never formed):
//   pmd_orthogonalize_factored: C = M^T (G M) -> Et (R' x m), rows = eigenvectors / sqrt(lambda)
//   pmd_projected_svd_factored: V = Et (M^T Z); SVD of V; R_out = M (Et^T W)
// =============================================================================================
extern "C" size_t pmd_orthogonalize_factored_workspace_bytes(int m) {
  return (size_t)m * m * sizeof(float) + (size_t)m * (3 * sizeof(float) + sizeof(int)) + 8192;
}

extern "C" int pmd_orthogonalize_factored(pmd_ctx* ctx, const float* M, int Rc, int m, long ldm, const float* GM,
                                          long ldgm, float* Et_out, long lde, int* rprime_out, void* ws,
                                          size_t ws_bytes) {
  CTX_CHECK(ctx);
  pmd_arena ar(ws, ws_bytes);
  float* C = ar.take_n<float>((size_t)m * m);
  const eig_bufs eb(ar, m, false);
  if (ar.overflow) return pmd_fail(ctx, PMD_ERR_WORKSPACE, "pmd_orthogonalize_factored", "workspace too small");
  RUN(pmd_gemm_rm(ctx, 1, 0, m, m, Rc, 1.f, M, ldm, GM, ldgm, 0.f, C, m));
  eig_host eh;
  RUN(eig_orthogonaliser(ctx, m, C, m, eb, eh, Et_out, lde, rprime_out));
  if (*rprime_out > 0) PMD_HIP(ctx, hipStreamSynchronize(ctx->stream));   // eh's vectors are host temporaries
  return PMD_OK;
}

extern "C" size_t pmd_projected_svd_factored_workspace_bytes(int Rc, int m, int rp, int T) {
  return (size_t)m * T * sizeof(float) + (size_t)rp * T * sizeof(float) + (size_t)m * rp * sizeof(float) +
         (size_t)m * pmd_round_up(Rc, 64) * sizeof(float) + pmd_projected_svd_workspace_bytes(1, rp, T) + 16384;
}

// M: Rc x m; Et: rp x m; Z: Rc x T.  Outputs R_out (Rc x nk), s (nk), Vt (nk x T), nk = min(rp, T);
// Vp_out (rp x T, optional, may be NULL) receives V = P^T Z.
extern "C" int pmd_projected_svd_factored(pmd_ctx* ctx, const float* M, int Rc, int m, long ldm, const float* Et,
                                          int rp, long lde, const float* Z, int T, long ldz, float* R_out, long ldr,
                                          float* s_out, float* Vt_out, long ldvt, float* Vp_out, long ldvp,
                                          float* X1_out, const float* W1_in, int et_lower, void* ws, size_t ws_bytes) {
  CTX_CHECK(ctx);
  if (rp > T) return pmd_fail(ctx, PMD_ERR_UNSUPPORTED, "pmd_projected_svd_factored", "needs R' <= T");
  pmd_arena ar(ws, ws_bytes);
  float* W1 = ar.take_n<float>((size_t)m * T);
  float* Vp = Vp_out ? Vp_out : ar.take_n<float>((size_t)rp * T);
  const long ldv = Vp_out ? ldvp : T;
  float* X1 = X1_out ? X1_out : ar.take_n<float>((size_t)m * rp);
  const long ldt = pmd_round_up(Rc, 64);   // (rows of the transposed copy on 256-byte boundaries, see pmd_gram_mtgm_ld)
  float* Mt = ar.take_n<float>((size_t)m * ldt);
  const size_t sub_bytes = pmd_projected_svd_workspace_bytes(1, rp, T);
  void* sub = ar.take(sub_bytes);
  if (ar.overflow) return pmd_fail(ctx, PMD_ERR_WORKSPACE, "pmd_projected_svd_factored", "workspace too small");
  // M^T Z as a plain (non-transposed) product of an explicit copy of M^T: rocBLAS' transposed-A kernels
  // reach half the rate of the plain ones at K = Rc ~ 5e4 (72 vs 147 TFLOP/s, scripts/gemm_probe.hip),
  // and the copy is one 2 x 4 Rc m byte pass
  if (!W1_in) {
    RUN(launch_transpose(ctx, M, ldm, Rc, m, Mt, ldt));
    RUN(pmd_gemm_rm(ctx, 0, 0, m, T, Rc, 1.f, Mt, ldt, Z, ldz, 0.f, W1, T));      // M^T Z
  }
  // (W1_in: the caller has formed M^T Z already, e.g. as an all-reduced sum of per-rank row-range partials)
  RUN(psvd_vp(ctx, Et, rp, m, lde, W1_in ? W1_in : W1, T, T, et_lower, Vp, ldv));     // V = Et (M^T Z)
  // SVD of V with the identity as projection: the "R" it returns is W (rp x rp), reuse W1's memory
  float* Wmat = W1;  // rp x rp  (rp <= m, T)
  RUN(pmd_projected_svd(ctx, nullptr, 0, 0, Vp, rp, T, ldv, Wmat, rp, s_out, Vt_out, ldvt, sub, sub_bytes));
  // R = M (Et^T W)
  if (et_lower && rp == m && !pmd_f16x2_wanted(ctx, m, rp, rp)) {
    // row-major X1 = Et^T W  <=>  column-major X1^T = W^T (Et^T)^T
    pmd_prof_scope prof__(ctx, "rocblas_strmm");
    const float one = 1.f;
    PMD_BLAS(ctx, rocblas_strmm(ctx->blas, rocblas_side_right, rocblas_fill_upper, rocblas_operation_transpose,
                                rocblas_diagonal_non_unit, rp, m, &one, Et, (rocblas_int)lde, Wmat, rp, X1, rp));
  } else {
    RUN(pmd_gemm_rm(ctx, 1, 0, m, rp, rp, 1.f, Et, lde, Wmat, rp, 0.f, X1, rp));
  }
  if (R_out) RUN(pmd_gemm_rm(ctx, 0, 0, Rc, rp, m, 1.f, M, ldm, X1, rp, 0.f, R_out, ldr));
  return PMD_OK;
}

extern "C" int pmd_transpose(pmd_ctx* ctx, const float* src, long lds_, int rows, int cols, float* dst, long ldd) {
  CTX_CHECK(ctx);
  return launch_transpose(ctx, src, lds_, rows, cols, dst, ldd);
}
