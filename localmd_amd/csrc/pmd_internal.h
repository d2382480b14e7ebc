// Launchers shared between the translation units of libpmd_hip.so.
#pragma once
#include "pmd_common.h"
#include "../../include/pmd_hip.h"   // the entry points: each is defined in the file that implements it

// rng.hip
int pmd_launch_rng(pmd_ctx* ctx, uint64_t seed, uint32_t stream, uint32_t index0, uint32_t index_step, int batch,
                   long rows, int cols, int transpose, float* out, long ld, long batch_stride);

// prep.hip
int pmd_init_tables(pmd_ctx* ctx);
int pmd_launch_tile_pool_bin(pmd_ctx* ctx, const float* X, long ldx, long n_rows, const int* pix, int n_tiles, int d,
                             const int* pool_q, int pool_max, int P, int a, int nbins, float* xbar, float* abar,
                             long ld_ab, long tile_stride);

// tile_gemm.hip
struct pmd_atx_opts {
  const char* label = "tile_atx";   // profile group of the launch
  int rows = 0;                     // rows of A that carry data (0: all 64)
  const int* ranks = nullptr;       // per-tile ranks (projection: rows >= rank of A are zero), or NULL
};
int pmd_launch_tile_atx(pmd_ctx* ctx, const float* X, long ldx, const int* pix, int pix_stride, long row0_stride, int d,
                        const float* A, long a_tile_stride, int a_ld, float* Out, long out_tile_stride, long ldo,
                        int n_tiles, int T, int slices, const pmd_atx_opts& opts = {});
int pmd_launch_tile_xbt(pmd_ctx* ctx, const float* X, long ldx, const int* pix, int pix_stride, long row0_stride, int d,
                        const float* B, long b_tile_stride, long ldb, float* S, long s_tile_stride,
                        long s_slice_stride, int s_ld, int n_tiles, int T, int slices);
int pmd_launch_tile_gram(pmd_ctx* ctx, const float* In, long tile_stride, long ld, int len, int n_tiles, int slices,
                         double* G);
int pmd_launch_gram_f2d(pmd_ctx* ctx, const float* in, int ld, long n_blocks, double* out);
int pmd_launch_reduce_slices(pmd_ctx* ctx, const float* in, long tile_stride, long slice_stride, int slices, long n,
                             float* out, long out_tile_stride, int n_tiles);
int pmd_launch_tile_rowmix(pmd_ctx* ctx, const float* In, long in_tile_stride, long ld_in, const double* N,
                           long n_tile_stride, int n_in, int n_out, float* Out, long out_tile_stride, long ld_out,
                           int len, int n_tiles);

// small_la.hip
bool pmd_small_qr_fits(int P, int l);
int pmd_launch_small_qr(pmd_ctx* ctx, const float* Yt, long y_tile_stride, int y_ld, int P, int l, float* Qt,
                        long q_tile_stride, int q_ld, int n_tiles);
int pmd_launch_small_eig(pmd_ctx* ctx, const double* G, int slices, int n, int mode, double tol, double* Nout,
                         double* lam_out, int n_tiles);
int pmd_launch_small_chol(pmd_ctx* ctx, const double* G, int slices, int n, double tol, double* Nout, int n_tiles);
int pmd_launch_expand_pooled(pmd_ctx* ctx, const float* In, long in_tile_stride, int in_ld, const int* pool_idx,
                             const float* pool_w, int d, int r, float* Out, long out_tile_stride, int out_ld,
                             int n_tiles);
int pmd_launch_stats_roughness(pmd_ctx* ctx, const float* Ut, long u_tile_stride, int u_ld, int b1, int b2,
                               const float* V, long v_tile_stride, long v_ld, int T, int r, float* stats, int n_tiles,
                               int rp);
int pmd_launch_decide(pmd_ctx* ctx, float* stats, int r, float thr_s, float thr_t, int max_fail, int cap,
                      int n_tiles, int* good, int* keep, int* ranks, int rp);

// wide.hip: generic-width forms of the small dense algebra (per-tile arrays [tile][rp][x], rp = pmd_tile_rpad(r) > 64),
// and the contractions in row blocks of 64 (any rp: nrows <= 64 is one launch of pmd_launch_tile_atx / _xbt)
int pmd_launch_wide_gram(pmd_ctx* ctx, const float* In, long tile_stride, long ld, int len, int n_tiles, int slices, int rp,
                         double* G, const float* In2 = nullptr);
size_t pmd_wide_eig_workspace_bytes(int n, int n_tiles);
int pmd_launch_wide_eig(pmd_ctx* ctx, const double* G, int slices, int rp, int n, int mode, double tol, double* Nout,
                        double* lam_out, int n_tiles, void* ws, size_t ws_bytes);
int pmd_launch_wide_rowmix(pmd_ctx* ctx, const float* In, long in_tile_stride, long ld_in, const double* N, long n_tile_stride,
                           int rp, int n_in, int n_out, float* Out, long out_tile_stride, long ld_out, int len, int n_tiles);
int pmd_launch_tile_atx_rp(pmd_ctx* ctx, const float* X, long ldx, const int* pix, int pix_stride, long row0_stride, int d,
                           const float* A, long a_tile_stride, int a_ld, float* Out, long out_tile_stride, long ldo, int n_tiles,
                           int T, int slices, int nrows, const pmd_atx_opts& opts = {});
int pmd_launch_tile_xbt_rp(pmd_ctx* ctx, const float* X, long ldx, const int* pix, int pix_stride, long row0_stride, int d,
                           const float* B, long b_tile_stride, long ldb, float* S, long s_tile_stride, long s_slice_stride, int s_ld,
                           int n_tiles, int T, int slices, int nrows);

// global.hip (also used by gram.hip and chol.hip)
#define PMD_BLAS(ctx, call)                                                     \
  do {                                                                          \
    rocblas_status s__ = (call);                                                \
    if (s__ != rocblas_status_success) return pmd_fail(ctx, PMD_ERR_BLAS, #call, rocblas_status_to_string(s__)); \
  } while (0)
int pmd_gemm_rm(pmd_ctx* ctx, int transA, int transB, int m, int n, int k, float alpha, const float* A, long lda,
                const float* B, long ldb, float beta, float* C, long ldc);
int pmd_gemm_k_chunk(const pmd_ctx* ctx, int k);   // length of one fp32 accumulation chain in a product of inner dimension k
int launch_gather_rows(pmd_ctx* ctx, const float* src, long lds_, const int* perm, const float* scale, int nrows,
                       int ncols, float* dst, long ldd);   // dst[c][x] = src[perm[c]][x] * scale[c]
int launch_transpose(pmd_ctx* ctx, const float* src, long lds_, int rows, int cols, float* dst, long ldd);

// gemm_f16x2.hip: fp32 products from two fp16 pieces per operand (X 2^-e = h1 + 2^-11 h2)
bool pmd_f16x2_wanted(const pmd_ctx* ctx, int m, int n, int k);
int pmd_gemm_f16x2(pmd_ctx* ctx, int transA, int transB, int m, int n, int k, float alpha, const float* A, long lda, const float* B, long ldb,
                   float beta, float* C, long ldc, int* done);
int pmd_f16x2_exponents(pmd_ctx* ctx, int count, const float* const* X, const int* rows, const int* cols, const long* ld, int* e_out,
                        int* usable);
int pmd_f16cat_a(pmd_ctx* ctx, const float* X, int rows, int kk, long ld, int e, _Float16* out, long ldo);
int pmd_f16cat_b(pmd_ctx* ctx, const float* X, int kk, int cols, long ld, int e, _Float16* out, long ldo);
int pmd_f16_plain_matmul(pmd_ctx* ctx, int m, int n, int k, float alpha, const _Float16* A, long lda, const _Float16* B, long ldb, float beta,
                         float* C, long ldc, int* done);
int pmd_split_scratch(pmd_ctx* ctx, size_t need, void** out);
void pmd_f16x2_destroy(pmd_ctx* ctx);

// sytrd.hip
int pmd_syevd(pmd_ctx* ctx, int n, float* A, long lda, float* w, float* work, int* info);
int pmd_ctx_scratch2(pmd_ctx* ctx, size_t bytes, void** out);   // grows ctx->scratch2 to at least `bytes`

// sytrd2.hip
size_t pmd_sy2sb_workspace_bytes_impl(int n);
int pmd_sy2sb_impl(pmd_ctx* ctx, int n, float* A, long lda, float* tau1, int* flag_host, void* ws, size_t ws_bytes);
int pmd_sb2st_apply_q2_impl(pmd_ctx* ctx, int n, const float* V2, const float* tau2, float* Z, long ldz, int nvec);
size_t pmd_sb2st_workspace_bytes_impl(int n);
int pmd_sb2st_impl(pmd_ctx* ctx, int n, const float* A, long lda, float* d, float* e, float** V2_out, float** tau2_out,
                   void* ws, size_t ws_bytes);

// prep.hip / small_la.hip: residual windows (single_residual_block_md)
int pmd_launch_bin_average(pmd_ctx* ctx, const float* X, long ldx, long n_rows, int a, int nbins, float* xbar, long ldb);
int pmd_launch_tile_cross_gram(pmd_ctx* ctx, const float* A, const float* B, long tile_stride, int ld, int len,
                               double* G, int n_tiles);
int pmd_launch_tile_residual_rows(pmd_ctx* ctx, const float* X, long ldx, const int* pix, int d, const float* E,
                                  int e_ld, const float* W, long w_ld, int r, int len, float* out, long out_ld,
                                  int n_tiles, int rp);
int pmd_launch_tile_sub(pmd_ctx* ctx, float* a, const float* b, long tile_stride, int ld, int len, int n_tiles, int rp);
int pmd_launch_tile_append(pmd_ctx* ctx, const float* stats, int r, float thr_s, float thr_t, int max_fail, int cap,
                           const float* Unew, float* Ucur, int ld, int* counts, int* good, int* keep, int n_tiles,
                           int rp);
