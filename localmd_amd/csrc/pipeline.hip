// Host-side sequencing of the per-tile decomposition, the threshold simulation and the
// background rSVD.  Everything is enqueued on ctx->stream inside a caller-provided workspace;
// nothing here allocates or synchronises.
#include "pmd_internal.h"
#include <algorithm>

extern "C" int pmd_tile_dpad(int d) {
  if (d > 65536) return -1;
  if (d > 1024) return (int)pmd_round_up(d, 1024);   // tile_atx splits the pixel axis over the grid in slices of 1024
  pmd_dvariant v;
  if (!pmd_pick_dvariant(d, &v)) return -1;
  return v.dpad;
}

extern "C" long pmd_time_ld(long t) { return pmd_round_up(t, 64) + PMD_LD_SLACK; }

static const int GRAM_SLICES = 4;
static const int XBT_SLICES = 4;

// ------------------------------------------------------------------------------------------
// The small dense algebra of a tile stage at either width: one method per row of the table in DESIGN.md section 4c.
// Per-tile arrays are [tile][rp][ld] (tile stride rp * ld), mixing matrices [tile][rp][rp].  rp == 64 (max_components +
// 10 <= 64) takes the 64-row kernels of tile_gemm.hip / small_la.hip, rp = pmd_tile_rpad(r) > 64 the generic-width ones
// of wide.hip.  The contractions over frames / pixels go through pmd_launch_tile_atx_rp / _xbt_rp at every width (one
// launch per block of 64 rows that carries data: exactly one at 64 rows).
// ------------------------------------------------------------------------------------------
struct tile_la {
  pmd_ctx* ctx;
  int rp;
  double *gpart, *nmat, *lam;   // Gram matrices [tile][slice][rp][rp], mixing matrices [tile][rp][rp], eigenvalues [tile][rp]
  void* eig_ws;                 // rp > 64 only: workspace of pmd_launch_wide_eig
  size_t eig_ws_bytes;

  bool wide() const { return rp > 64; }

  // gpart = In In^T over `slices` slices of the positions; with In2, nmat = the cross Gram matrix In In2^T (one slice)
  int gram(const float* In, long ld, int len, int n, int slices, const float* In2 = nullptr) const {
    if (wide()) return pmd_launch_wide_gram(ctx, In, rp * ld, ld, len, n, slices, rp, In2 ? nmat : gpart, In2);
    if (In2) return pmd_launch_tile_cross_gram(ctx, In, In2, rp * ld, (int)ld, len, nmat, n);
    return pmd_launch_tile_gram(ctx, In, rp * ld, ld, len, n, slices, gpart);
  }

  // nmat = eigenvectors of the summed leading n x n blocks of gpart, by descending eigenvalue (mode 1: scaled by
  // 1/sqrt(lambda), directions with lambda <= tol * lambda_max zeroed; mode 2: those directions zeroed, no scaling)
  int eig(int slices, int n, int mode, double tol, double* lam_out, int n_tiles) const {
    if (wide()) return pmd_launch_wide_eig(ctx, gpart, slices, rp, n, mode, tol, nmat, lam_out, n_tiles, eig_ws, eig_ws_bytes);
    return pmd_launch_small_eig(ctx, gpart, slices, n, mode, tol, nmat, lam_out, n_tiles);
  }

  // nmat = a matrix that orthonormalises the rows whose Gram matrix is in gpart.  Where only the span matters downstream
  // (chol_allowed) the 64-row path takes the Cholesky form (small_la.hip); the generic-width path has eigen-whitening only.
  int whiten(int slices, int n, double tol, bool chol_allowed, int n_tiles) const {
    if (!wide() && chol_allowed) return pmd_launch_small_chol(ctx, gpart, slices, n, tol, nmat, n_tiles);
    return eig(slices, n, 1, tol, lam, n_tiles);
  }

  // Out[tile][c][x] = sum_c' nmat[tile][c'][c] In[tile][c'][x] (in-place safe); shared: one mixing matrix for all tiles
  int rowmix(const float* In, long ld_in, int n_in, int n_out, float* Out, long ld_out, int len, int n, bool shared = false) const {
    const long ns = shared ? 0 : (long)rp * rp;
    if (wide()) return pmd_launch_wide_rowmix(ctx, In, rp * ld_in, ld_in, nmat, ns, rp, n_in, n_out, Out, rp * ld_out, ld_out, len, n);
    return pmd_launch_tile_rowmix(ctx, In, rp * ld_in, ld_in, nmat, ns, n_in, n_out, Out, rp * ld_out, ld_out, len, n);
  }

  // Orthonormal basis Qt (nref rows) of the span of the l sketch rows Yt [l][P] (jnp.linalg.qr at decomposition.py:64 /
  // pmd_loader.py:58).  64 rows: Householder QR in LDS while the P x l matrix fits a workgroup's 160 KB (every default
  // configuration); beyond that - large tiles with spatial_avg_factor = 1 and a wide sketch, e.g. 30 x 40 pixels x 58
  // columns - CholeskyQR2: the same Q up to the signs of its columns (QR is unique up to them).  Wider: two rounds of
  // Gram matrix -> eigen-whitening -> row mixing, which sees all l rows in the first round (the Cholesky form pivots in
  // order and takes the leading nref).  Any orthonormal basis of the sketch's span serves the rSVD: B = Q^T A, the SVD of
  // B and U = Q W are invariant under Q -> Q O.
  int sketch_basis(const float* Yt, int ld, int P, int l, int nref, float* Qt, int n) const {
    if (!wide() && pmd_small_qr_fits(P, l)) return pmd_launch_small_qr(ctx, Yt, (long)rp * ld, ld, P, l, Qt, (long)rp * ld, ld, n);
    const float* src = Yt;
    for (int pass = 0; pass < 2; ++pass) {
      const int n_in = (wide() && pass == 0) ? l : nref;
      RUN(gram(src, ld, P, n, 1));
      RUN(whiten(1, n_in, 1e-12, true, n));
      RUN(rowmix(src, ld, n_in, nref, Qt, ld, P, n));
      src = Qt;
    }
    return PMD_OK;
  }
};

// the scratch of tile_la for n tiles, as the last allocations of a plan
static void take_la_scratch(pmd_arena& ar, tile_la& la, int rp_, size_t n) {
  const size_t rp = rp_;
  la.ctx = nullptr;   // the entry point that runs the plan sets it
  la.rp = rp_;
  la.gpart = ar.take_n<double>(n * GRAM_SLICES * rp * rp);
  la.nmat = ar.take_n<double>(n * rp * rp);
  la.lam = ar.take_n<double>(n * rp);
  la.eig_ws = nullptr;
  la.eig_ws_bytes = 0;
  if (la.wide()) {
    la.eig_ws_bytes = pmd_wide_eig_workspace_bytes(rp_, (int)n);
    la.eig_ws = ar.take(la.eig_ws_bytes);
  }
}

// Omega^T of the rSVD sketch of n tiles ([tile][rp][ld], l rows of nb columns drawn), in launch chunks of 32768 tiles
static int draw_tile_omega(pmd_ctx* ctx, uint64_t seed, uint32_t index0, uint32_t index_step, int n, int nb, int l, float* omT, long ld,
                           long tile_stride) {
  for (int t0 = 0; t0 < n; t0 += 32768) {
    const int tn = (n - t0 < 32768) ? n - t0 : 32768;
    RUN(pmd_launch_rng(ctx, seed, PMD_STREAM_TILE_OMEGA, index0 + (uint32_t)t0 * index_step, index_step, tn, nb, l, 1,
                       omT + (long)t0 * tile_stride, ld, tile_stride));
  }
  return PMD_OK;
}

// ------------------------------------------------------------------------------------------
// per-tile decomposition (decomposition.py:235-330 single_block_md, one window, + :501-523)
// ------------------------------------------------------------------------------------------
struct tiles_plan {
  int nb, l, dpad, Ppad, nref, rp;
  long ld_b;
  float *abar, *omT, *yt, *qt, *bm, *udst, *ut0, *outA, *spart, *sst, *xbar, *g1f;
  tile_la la;
  size_t zero_bytes;  // leading part of the workspace that must be zeroed
};

// rp = component rows of every per-tile array: 64 on the main path (max_components + 10 <= 64), pmd_tile_rpad(r) beyond
static int plan_tiles(pmd_arena& ar, tiles_plan& p, int n, int d, int P, int r, int a, int t_crop, long ldv, long n_rows) {
  p.nb = t_crop / a;
  p.l = r + 10;
  p.rp = pmd_tile_rpad(r);
  const size_t rp = p.rp;
  const bool wide = p.rp > 64;
  p.dpad = pmd_tile_dpad(d);
  p.Ppad = pmd_tile_dpad(P);
  p.nref = (P < p.l) ? P : p.l;
  p.ld_b = pmd_time_ld(p.nb);
  if (p.dpad < 0 || p.Ppad < 0) return PMD_ERR_UNSUPPORTED;
  // arrays with padding that is read before it is written come first (they get zeroed)
  p.abar = ar.take_n<float>((size_t)n * P * p.ld_b);
  p.omT = ar.take_n<float>((size_t)n * rp * p.ld_b);
  p.yt = ar.take_n<float>((size_t)n * rp * p.Ppad);
  p.qt = ar.take_n<float>((size_t)n * rp * p.Ppad);
  p.udst = ar.take_n<float>((size_t)n * rp * p.Ppad);
  p.ut0 = ar.take_n<float>((size_t)n * rp * p.dpad);
  p.spart = wide ? nullptr : ar.take_n<float>((size_t)n * XBT_SLICES * 64 * p.dpad);   // (the wide path runs S = X V^T in one slice)
  p.sst = ar.take_n<float>((size_t)n * rp * p.dpad);
  p.zero_bytes = ar.used;
  p.bm = ar.take_n<float>((size_t)n * rp * p.ld_b);
  p.xbar = ar.take_n<float>((size_t)n_rows * p.ld_b);
  p.g1f = wide ? nullptr : ar.take_n<float>((size_t)n * GRAM_SLICES * 4096);
  p.outA = ar.take_n<float>((size_t)n * rp * ldv);
  take_la_scratch(ar, p.la, p.rp, n);
  return PMD_OK;
}

extern "C" size_t pmd_tiles_workspace_bytes(int n, int b1, int b2, int P, int r, int a, int t_crop, long ldv,
                                            long n_rows) {
  const int d = b1 * b2;
  pmd_arena ar((void*)0x1000, ~size_t(0) >> 1);
  tiles_plan p;
  if (plan_tiles(ar, p, n, d, P, r, a, t_crop, ldv, n_rows) != PMD_OK) return 0;
  return ar.used + 4096;
}

extern "C" int pmd_tiles_decompose_staged(pmd_ctx* ctx, const float* Xf, long ldx, long n_rows, int t_crop,
                                          const int* tile_pix, int n, int b1, int b2, const int* pool_q, int pool_max,
                                          int P, const int* pool_idx, const float* pool_w, int r, int a, float thr_s,
                                          float thr_t, int max_fail, uint64_t seed, uint32_t omega_index0,
                                          uint32_t omega_index_step, float* Ut_out, float* V_out, long ldv,
                                          float* stats_out, int* good_out, int* keep_out, int* ranks_out,
                                          double* sing_out, void* ws, size_t ws_bytes, int stages) {
  CTX_CHECK(ctx);
  if (stages < 1 || stages > 7) return pmd_fail(ctx, PMD_ERR_ARG, "pmd_tiles_decompose_staged", "stages must be a mask of bits 0..2");
  const int d = b1 * b2;
  if (r < 1) return pmd_fail(ctx, PMD_ERR_ARG, "pmd_tiles_decompose", "max_components must be >= 1");
  if (a < 1 || t_crop % a != 0 || t_crop / a < 1) return pmd_fail(ctx, PMD_ERR_ARG, "pmd_tiles_decompose", "t_crop must be a positive multiple of temporal_avg_factor");
  if (ldv < pmd_time_ld(t_crop) || ldx < pmd_time_ld(t_crop)) return pmd_fail(ctx, PMD_ERR_ARG, "pmd_tiles_decompose", "leading dimension too small");
  pmd_arena ar(ws, ws_bytes);
  tiles_plan p;
  if (plan_tiles(ar, p, n, d, P, r, a, t_crop, ldv, n_rows) != PMD_OK)
    return pmd_fail(ctx, PMD_ERR_UNSUPPORTED, "pmd_tiles_decompose", "tile too large (max 65536 pixels)");
  if (ar.overflow) return pmd_fail(ctx, PMD_ERR_WORKSPACE, "pmd_tiles_decompose", "workspace too small");
  // max_components beyond the number of time bins or of pooled pixels: the reference's rSVD (decomposition.py:59-73) keeps
  // its sketch of max_components + 10 columns and `u_final[:, :rank]` simply returns the min(rank, bins, pixels) columns
  // that exist; everything downstream then works on that many components
  if (r > p.nb) r = p.nb;
  if (r > p.nref) r = p.nref;
  tile_la& la = p.la;
  la.ctx = ctx;
  const int rp = p.rp;
  const bool wide = la.wide();
  const long srd = (long)rp * p.dpad, srP = (long)rp * p.Ppad, srb = (long)rp * p.ld_b, srv = (long)rp * ldv;
  // Only spans matter at the two whitening steps, so the 64-row path may take the Cholesky form (the generic-width path
  // has none).  PMD_TILE_WHITEN=eig restores the eigenvector form (A/B runs).
  const bool whiten_chol_u0 = !ctx->routes.tile_whiten_eig;
  const bool whiten_chol = whiten_chol_u0 && stages == 7;   // the spatial_denoiser hook sees S = X V_b^T column by column
  // Time slices of the two contractions over all frames: four per tile give a few thousand tiles enough workgroups to fill
  // the chip; with many tiles (the 16 x 16-pixel regime: 16 129 / 65 025 tiles) one slice does, and the partial results
  // and their reduction pass (10 of 300 ms at 1024 x 1024 x 1000, b = 16) disappear.  The generic-width path, sized for
  // correctness and not tuned, always runs S in one slice and its Gram matrices in four.
  const int xs = (wide || n >= 4096) ? 1 : XBT_SLICES;
  const int gs = (!wide && n >= 4096) ? 1 : GRAM_SLICES;

  // stages: bit 0 = up to V_ds (p.outA; the temporal_denoiser hook of decomposition.py:300 acts on it),
  //         bit 1 = basis of its row space and S = X V_b^T (p.sst; spatial_denoiser hook, :310), bit 2 = the rest
  if (stages & 1) {
    PMD_HIP(ctx, hipMemsetAsync(ws, 0, p.zero_bytes, ctx->stream));
    PMD_HIP(ctx, hipMemsetAsync(Ut_out, 0, (size_t)n * srd * sizeof(float), ctx->stream));

    // --- rSVD of the pooled, temporally binned tile (decomposition.py:279-294, :59-73)
    RUN(pmd_launch_tile_pool_bin(ctx, Xf, ldx, n_rows, tile_pix, n, d, pool_q, pool_max, P, a, p.nb, p.xbar, p.abar, p.ld_b, (long)P * p.ld_b));
    RUN(draw_tile_omega(ctx, seed, omega_index0, omega_index_step, n, p.nb, p.l, p.omT, p.ld_b, srb));
    RUN(pmd_launch_tile_xbt_rp(ctx, p.abar, p.ld_b, nullptr, 0, P, P, p.omT, srb, p.ld_b, p.yt, srP, 0, p.Ppad, n, p.nb, 1, p.l));
    RUN(la.sketch_basis(p.yt, p.Ppad, P, p.l, p.nref, p.qt, n));
    RUN(pmd_launch_tile_atx_rp(ctx, p.abar, p.ld_b, nullptr, 0, P, P, p.qt, srP, p.Ppad, p.bm, srb, p.ld_b, n, p.nb, 1, p.nref));
    RUN(la.gram(p.bm, p.ld_b, p.nb, n, 1));
    RUN(la.eig(1, p.nref, 0, 0.0, la.lam, n));
    RUN(la.rowmix(p.qt, p.Ppad, p.nref, r, p.udst, p.Ppad, P, n));
    RUN(pmd_launch_expand_pooled(ctx, p.udst, srP, p.Ppad, pool_idx, pool_w, d, r, p.ut0, srd, p.dpad, n));

    // --- V_ds = U_ds^T X_ds; basis of its row space (decomposition.py:295-301)
    RUN(pmd_launch_tile_atx_rp(ctx, Xf, ldx, tile_pix, d, 0, d, p.ut0, srd, p.dpad, p.outA, srv, ldv, n, t_crop, 2, r, {"tile_atx_main"}));
  }
  if (stages & 2) {
    if (wide) {
      RUN(la.gram(p.outA, ldv, t_crop, n, gs));
    } else {
      // (this Gram only conditions the basis change -- span(S) does not depend on it -- so fp32 MFMA is enough)
      RUN(pmd_launch_tile_xbt(ctx, p.outA, ldv, nullptr, 0, 64, 64, p.outA, srv, ldv, p.g1f, gs * 4096L, 4096, 64, n, t_crop, gs));
      RUN(pmd_launch_gram_f2d(ctx, p.g1f, 64, (long)n * gs, la.gpart));
    }
    // only span(S) matters downstream: with no denoiser hook reading S component by component (stages == 7) any orthonormal
    // basis of the row space of V_ds serves
    RUN(la.whiten(gs, r, 1e-10, whiten_chol, n));

    // --- S = X V_b^T and its left singular vectors U0 (decomposition.py:304-317)
    if (xs == 1) {
      RUN(pmd_launch_tile_xbt_rp(ctx, Xf, ldx, tile_pix, d, 0, d, p.outA, srv, ldv, p.sst, srd, 0, p.dpad, n, t_crop, 1, r));
    } else {
      RUN(pmd_launch_tile_xbt_rp(ctx, Xf, ldx, tile_pix, d, 0, d, p.outA, srv, ldv, p.spart, xs * srd, srd, p.dpad, n, t_crop, xs, r));
      RUN(pmd_launch_reduce_slices(ctx, p.spart, xs * srd, srd, xs, srd, p.sst, srd, n));
    }
    RUN(la.rowmix(p.sst, p.dpad, r, r, p.sst, p.dpad, d, n));
  }
  if (stages & 4) {
    RUN(la.gram(p.sst, p.dpad, d, n, 1));
    // U = U0 Wl depends on span(U0) = span(S) only: an orthonormal basis of it is enough (always; no hook reads U0)
    RUN(la.whiten(1, r, 1e-10, whiten_chol_u0, n));
    RUN(la.rowmix(p.sst, p.dpad, r, r, p.sst, p.dpad, d, n));

    // --- W = U0^T X, its SVD rotates U0 and gives sigma*V (decomposition.py:318-323)
    RUN(pmd_launch_tile_atx_rp(ctx, Xf, ldx, tile_pix, d, 0, d, p.sst, srd, p.dpad, V_out, srv, ldv, n, t_crop, 2, r, {"tile_atx_main"}));
    RUN(la.gram(V_out, ldv, t_crop, n, gs));
    RUN(la.eig(gs, r, 0, 0.0, sing_out ? sing_out : la.lam, n));
    RUN(la.rowmix(p.sst, p.dpad, r, r, Ut_out, p.dpad, d, n));
    RUN(la.rowmix(V_out, ldv, r, r, V_out, ldv, t_crop, n));

    // --- roughness statistics and keep/discard scan (evaluation.py:84-222)
    RUN(pmd_launch_stats_roughness(ctx, Ut_out, srd, p.dpad, b1, b2, V_out, srv, ldv, t_crop, r, stats_out, n, rp));
    RUN(pmd_launch_decide(ctx, stats_out, r, thr_s, thr_t, max_fail, r, n, good_out, keep_out, ranks_out, rp));
  }
  return PMD_OK;
}

extern "C" int pmd_tiles_decompose(pmd_ctx* ctx, const float* xf, long ldx, long n_rows, int t_crop, const int* tile_pix, int n_tiles,
                                   int b1, int b2, const int* pool_q, int pool_max, int P, const int* pool_idx, const float* pool_w,
                                   int r, int a, float thr_s, float thr_t, int max_fail, uint64_t seed, uint32_t omega_index0,
                                   uint32_t omega_index_step, float* Ut_out, float* V_out, long ldv, float* stats_out, int* good_out,
                                   int* keep_out, int* ranks_out, double* lam_out, void* ws, size_t ws_bytes) {
  return pmd_tiles_decompose_staged(ctx, xf, ldx, n_rows, t_crop, tile_pix, n_tiles, b1, b2, pool_q, pool_max, P, pool_idx, pool_w, r,
                                    a, thr_s, thr_t, max_fail, seed, omega_index0, omega_index_step, Ut_out, V_out, ldv, stats_out,
                                    good_out, keep_out, ranks_out, lam_out, ws, ws_bytes, 7);
}

extern "C" int pmd_tiles_hook_offsets(int n, int b1, int b2, int P, int r, int a, int t_crop, long ldv, long n_rows,
                                      size_t* vds_off, size_t* s_off) {
  if (!vds_off || !s_off) return PMD_ERR_ARG;
  const int d = b1 * b2;
  pmd_arena ar((void*)0x1000, ~size_t(0) >> 1);
  tiles_plan p;
  if (plan_tiles(ar, p, n, d, P, r, a, t_crop, ldv, n_rows) != PMD_OK) return PMD_ERR_UNSUPPORTED;
  *vds_off = (size_t)((char*)p.outA - (char*)0x1000);
  *s_off = (size_t)((char*)p.sst - (char*)0x1000);
  return PMD_OK;
}

// ------------------------------------------------------------------------------------------
// residual window (decomposition.py:333-387 single_residual_block_md + :501-515): components of the
// part of the window that the current basis E does not explain.  (I - E E^T) commutes with the
// temporal bin average, so the residual is never materialised at full resolution.
// ------------------------------------------------------------------------------------------
struct resid_plan {
  int nb, l, dpad, nref, rp;
  long ld_b, ld_L;
  float *xbar, *wbar, *ar, *omT, *yt, *qt, *bm, *unew, *tmp, *util, *vmat;
  tile_la la;
  size_t zero_bytes;
};

static int plan_resid(pmd_arena& ar, resid_plan& p, int n, int d, int r, int a, int L, long n_rows) {
  p.nb = L / a;
  p.l = r + 10;
  p.rp = pmd_tile_rpad(r);
  const size_t rp = p.rp;
  p.dpad = pmd_tile_dpad(d);
  if (p.dpad < 0) return PMD_ERR_UNSUPPORTED;
  p.nref = d < p.l ? d : p.l;
  p.ld_b = pmd_time_ld(p.nb);
  p.ld_L = pmd_time_ld(L);
  p.omT = ar.take_n<float>((size_t)n * rp * p.ld_b);
  p.ar = ar.take_n<float>((size_t)n * d * p.ld_b);
  p.yt = ar.take_n<float>((size_t)n * rp * p.dpad);
  p.qt = ar.take_n<float>((size_t)n * rp * p.dpad);
  p.unew = ar.take_n<float>((size_t)n * rp * p.dpad);
  p.tmp = ar.take_n<float>((size_t)n * rp * p.dpad);
  p.util = ar.take_n<float>((size_t)n * rp * p.dpad);
  p.zero_bytes = ar.used;
  p.xbar = ar.take_n<float>((size_t)n_rows * p.ld_b);
  p.wbar = ar.take_n<float>((size_t)n * rp * p.ld_b);
  p.bm = ar.take_n<float>((size_t)n * rp * p.ld_b);
  p.vmat = ar.take_n<float>((size_t)n * rp * p.ld_L);
  take_la_scratch(ar, p.la, p.rp, n);
  return PMD_OK;
}

extern "C" size_t pmd_tiles_residual_workspace_bytes(int n, int b1, int b2, int r, int a, int L, long n_rows) {
  const int d = b1 * b2;
  pmd_arena ar((void*)0x1000, ~size_t(0) >> 1);
  resid_plan p;
  if (plan_resid(ar, p, n, d, r, a, L, n_rows) != PMD_OK) return 0;
  return ar.used + 4096;
}

extern "C" int pmd_tiles_residual(pmd_ctx* ctx, const float* Xw, long ldx, long n_rows, int L, const int* tile_pix,
                                  int n, int b1, int b2, int r, int a, float thr_s, float thr_t, int max_fail,
                                  uint64_t seed, uint32_t omega_index0, uint32_t omega_index_step, float* Ucur,
                                  int* counts, float* stats_out, int* good_out, int* keep_out, void* ws,
                                  size_t ws_bytes) {
  CTX_CHECK(ctx);
  const int d = b1 * b2;
  if (r < 1) return pmd_fail(ctx, PMD_ERR_ARG, "pmd_tiles_residual", "max_components must be >= 1");
  if (a < 1 || L % a != 0 || L / a < 1) return pmd_fail(ctx, PMD_ERR_ARG, "pmd_tiles_residual", "window length must be a positive multiple of temporal_avg_factor");
  if (ldx < pmd_time_ld(L)) return pmd_fail(ctx, PMD_ERR_ARG, "pmd_tiles_residual", "leading dimension too small");
  pmd_arena ar(ws, ws_bytes);
  resid_plan p;
  if (plan_resid(ar, p, n, d, r, a, L, n_rows) != PMD_OK) return pmd_fail(ctx, PMD_ERR_UNSUPPORTED, "pmd_tiles_residual", "tile too large");
  if (ar.overflow) return pmd_fail(ctx, PMD_ERR_WORKSPACE, "pmd_tiles_residual", "workspace too small");
  tile_la& la = p.la;
  la.ctx = ctx;
  const int rp = p.rp;
  const long srd = (long)rp * p.dpad, srb = (long)rp * p.ld_b, srL = (long)rp * p.ld_L;
  PMD_HIP(ctx, hipMemsetAsync(ws, 0, p.zero_bytes, ctx->stream));

  // A_r = (I - E E^T) binavg(X_window)
  RUN(pmd_launch_bin_average(ctx, Xw, ldx, n_rows, a, p.nb, p.xbar, p.ld_b));
  RUN(pmd_launch_tile_atx_rp(ctx, p.xbar, p.ld_b, tile_pix, d, 0, d, Ucur, srd, p.dpad, p.wbar, srb, p.ld_b, n, p.nb, 1, r));
  RUN(pmd_launch_tile_residual_rows(ctx, p.xbar, p.ld_b, tile_pix, d, Ucur, p.dpad, p.wbar, p.ld_b, r, p.nb, p.ar, p.ld_b, n, rp));
  // rSVD of A_r (decomposition.py:378, :59-73)
  RUN(draw_tile_omega(ctx, seed, omega_index0, omega_index_step, n, p.nb, p.l, p.omT, p.ld_b, srb));
  RUN(pmd_launch_tile_xbt_rp(ctx, p.ar, p.ld_b, nullptr, 0, d, d, p.omT, srb, p.ld_b, p.yt, srd, 0, p.dpad, n, p.nb, 1, p.l));
  RUN(la.sketch_basis(p.yt, p.dpad, d, p.l, p.nref, p.qt, n));
  RUN(pmd_launch_tile_atx_rp(ctx, p.ar, p.ld_b, nullptr, 0, d, d, p.qt, srd, p.dpad, p.bm, srb, p.ld_b, n, p.nb, 1, p.nref));
  RUN(la.gram(p.bm, p.ld_b, p.nb, n, 1));
  // A direction the residual does not have (lambda <= 1e-10 lambda_max, the cut of the first window's whitening; every
  // direction of an all-zero residual) gets a zero vector, not the arbitrary unit vector the QR of the sketch leaves there:
  // such a vector is not orthogonal to E.  Its statistics are 0 / 0, it fails, and the scan keeps it like any other failure.
  RUN(la.eig(1, p.nref, 2, 1e-10, la.lam, n));
  // new components of this window: min(max_components, bins, pixels) of them exist (see pmd_tiles_decompose_staged)
  const int rn = std::min(r, std::min(p.nb, p.nref));
  RUN(la.rowmix(p.qt, p.dpad, p.nref, rn, p.unew, p.dpad, d, n));
  // v = u^T (I - E E^T) X = utilde^T X with utilde = u - E (E^T u)   (decomposition.py:370-371, :379): the cross Gram
  // matrix E^T u is the mixing matrix of the row mix of E
  RUN(la.gram(Ucur, p.dpad, d, n, 1, p.unew));
  RUN(la.rowmix(Ucur, p.dpad, r, rn, p.tmp, p.dpad, d, n));
  PMD_HIP(ctx, hipMemcpyAsync(p.util, p.unew, (size_t)n * srd * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  RUN(pmd_launch_tile_sub(ctx, p.util, p.tmp, srd, p.dpad, d, n, rp));
  RUN(pmd_launch_tile_atx_rp(ctx, Xw, ldx, tile_pix, d, 0, d, p.util, srd, p.dpad, p.vmat, srL, p.ld_L, n, L, 2, rn));
  // fitness, keep/discard scan, append behind the existing components
  RUN(pmd_launch_stats_roughness(ctx, p.unew, srd, p.dpad, b1, b2, p.vmat, srL, p.ld_L, L, rn, stats_out, n, rp));
  RUN(pmd_launch_tile_append(ctx, stats_out, rn, thr_s, thr_t, max_fail, r, p.unew, Ucur, p.dpad, counts, good_out, keep_out, n, rp));
  return PMD_OK;
}

// ------------------------------------------------------------------------------------------
// threshold simulation (decomposition.py:76-131, :147-181): rank-1 rSVD of N(0,1) tiles
// ------------------------------------------------------------------------------------------
static const int SIM_BATCH = 256;  // one batch for the reference's 250 iterations (~22 MB of workspace each)

struct sim_plan {
  int dpad, nbatch;
  long ld_t;
  float *yt, *ypart, *qt, *ut, *noise, *omT, *bm, *stats;
  tile_la la;   // always 64 rows: a sketch of 11 columns
  size_t zero_bytes;
};

static int plan_sim(pmd_arena& ar, sim_plan& p, int d, int t, int iters) {
  p.dpad = pmd_tile_dpad(d);
  if (p.dpad < 0) return PMD_ERR_UNSUPPORTED;
  p.nbatch = iters < SIM_BATCH ? iters : SIM_BATCH;
  p.ld_t = pmd_time_ld(t);
  const size_t nb = p.nbatch;
  p.ypart = ar.take_n<float>(nb * XBT_SLICES * 64 * p.dpad);
  p.yt = ar.take_n<float>(nb * 64 * p.dpad);
  p.qt = ar.take_n<float>(nb * 64 * p.dpad);
  p.ut = ar.take_n<float>(nb * 64 * p.dpad);
  p.omT = ar.take_n<float>(nb * 64 * p.ld_t);
  p.noise = ar.take_n<float>(nb * d * p.ld_t);
  p.zero_bytes = ar.used;
  p.bm = ar.take_n<float>(nb * 64 * p.ld_t);
  p.stats = ar.take_n<float>(nb * 64 * 2);
  take_la_scratch(ar, p.la, 64, nb);
  return PMD_OK;
}

extern "C" size_t pmd_threshold_sim_workspace_bytes(int b1, int b2, int t, int iters) {
  const int d = b1 * b2;
  pmd_arena ar((void*)0x1000, ~size_t(0) >> 1);
  sim_plan p;
  if (plan_sim(ar, p, d, t, iters) != PMD_OK) return 0;
  return ar.used + 4096;
}

__global__ void copy_sim_stats_kernel(const float* __restrict__ stats, int nb, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb) {
    out[2 * i + 0] = stats[(long)i * PMD_RPAD * 2 + 0];
    out[2 * i + 1] = stats[(long)i * PMD_RPAD * 2 + 1];
  }
}

extern "C" int pmd_threshold_sim(pmd_ctx* ctx, int b1, int b2, int t, int iters, uint64_t seed, float* stats_out,
                                 void* ws, size_t ws_bytes) {
  CTX_CHECK(ctx);
  const int d = b1 * b2;
  const int l = 11;  // num_comps = 1, ten oversamples (decomposition.py:59, :708)
  if (t < 3) return pmd_fail(ctx, PMD_ERR_ARG, "pmd_threshold_sim", "need at least 3 frames");
  pmd_arena ar(ws, ws_bytes);
  sim_plan p;
  if (plan_sim(ar, p, d, t, iters) != PMD_OK) return pmd_fail(ctx, PMD_ERR_UNSUPPORTED, "pmd_threshold_sim", "tile too large");
  if (ar.overflow) return pmd_fail(ctx, PMD_ERR_WORKSPACE, "pmd_threshold_sim", "workspace too small");
  tile_la& la = p.la;
  la.ctx = ctx;
  const long s64d = 64L * p.dpad, s64t = 64L * p.ld_t;
  const int nref = d < l ? d : l;
  for (int it0 = 0; it0 < iters; it0 += p.nbatch) {
    const int nb = (iters - it0 < p.nbatch) ? iters - it0 : p.nbatch;
    PMD_HIP(ctx, hipMemsetAsync(ws, 0, p.zero_bytes, ctx->stream));
    RUN(pmd_launch_rng(ctx, seed, PMD_STREAM_SIM_NOISE, (uint32_t)it0, 1, nb, d, t, 0, p.noise, p.ld_t, (long)d * p.ld_t));
    RUN(pmd_launch_rng(ctx, seed, PMD_STREAM_SIM_OMEGA, (uint32_t)it0, 1, nb, t, l, 1, p.omT, p.ld_t, s64t));
    RUN(pmd_launch_tile_xbt(ctx, p.noise, p.ld_t, nullptr, 0, d, d, p.omT, s64t, p.ld_t, p.ypart, XBT_SLICES * s64d, s64d, p.dpad, nb, t, XBT_SLICES));
    RUN(pmd_launch_reduce_slices(ctx, p.ypart, XBT_SLICES * s64d, s64d, XBT_SLICES, s64d, p.yt, s64d, nb));
    RUN(la.sketch_basis(p.yt, p.dpad, d, l, nref, p.qt, nb));
    RUN(pmd_launch_tile_atx(ctx, p.noise, p.ld_t, nullptr, 0, d, d, p.qt, s64d, p.dpad, p.bm, s64t, p.ld_t, nb, t, 4));
    RUN(la.gram(p.bm, p.ld_t, t, nb, GRAM_SLICES));
    RUN(la.eig(GRAM_SLICES, nref, 0, 0.0, la.lam, nb));
    RUN(la.rowmix(p.qt, p.dpad, nref, 1, p.ut, p.dpad, d, nb));
    RUN(la.rowmix(p.bm, p.ld_t, nref, 1, p.bm, p.ld_t, t, nb));
    RUN(pmd_launch_stats_roughness(ctx, p.ut, s64d, p.dpad, b1, b2, p.bm, s64t, p.ld_t, t, 1, p.stats, nb, 64));
    hipLaunchKernelGGL(copy_sim_stats_kernel, dim3((nb + 63) / 64), dim3(64), 0, ctx->stream, p.stats, nb, stats_out + 2L * it0);
    PMD_LAUNCH_CHECK(ctx, "copy_sim_stats_kernel");
  }
  return PMD_OK;
}

// ------------------------------------------------------------------------------------------
// background basis (pmd_loader.py:46-68, :300-314): rSVD of the standardised sample, with the
// tall-skinny QR done as CholeskyQR2 in fp64 (Q differs from Householder's by column signs
// only, which cancel in U = Q u).
// ------------------------------------------------------------------------------------------
#define BG_BLK 256

__global__ void sum_gram_blocks_kernel(const double* __restrict__ g, int nblk, double* __restrict__ out, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += g[(long)b * count + i];
  out[i] = s;
}

// G = R^T R (upper R); N[c'][c] = (R^{-1})[c'][c].  Pivots <= tol * max diagonal give a zero column.
__global__ __launch_bounds__(64) void chol_inverse_kernel(const double* __restrict__ G, int n, double tol,
                                                          double* __restrict__ N) {
  __shared__ double R[64][65];
  __shared__ double Ri[64][65];
  __shared__ int dead[64];
  const int t = threadIdx.x;
  for (int i = 0; i < 64; ++i) { R[i][t] = (i < n && t < n) ? 0.5 * (G[i * 64 + t] + G[t * 64 + i]) : 0.0; Ri[i][t] = 0.0; }
  __syncthreads();
  double dmax = 0.0;
  for (int i = 0; i < n; ++i) dmax = fmax(dmax, R[i][i]);
  // right-looking Cholesky, upper factor stored in R (row k = R[k][k:])
  for (int k = 0; k < n; ++k) {
    const double piv = R[k][k];
    const bool bad = !(piv > tol * dmax);
    if (t == 0) dead[k] = bad;
    __syncthreads();
    const double rkk = bad ? 1.0 : sqrt(piv);
    double rkt = 0.0;
    if (t >= k && t < n) rkt = bad ? ((t == k) ? 1.0 : 0.0) : R[k][t] / rkk;
    __syncthreads();
    if (t >= k && t < n) R[k][t] = rkt;
    __syncthreads();
    if (!bad) {
      // trailing update: R[i][j] -= R[k][i] * R[k][j], i,j > k ; thread t owns column j = t
      if (t > k && t < n)
        for (int i = k + 1; i <= t; ++i) R[i][t] -= R[k][i] * R[k][t];
    }
    __syncthreads();
  }
  // invert the upper-triangular factor: thread t solves column t of R * X = I
  if (t < n) {
    for (int i = t; i >= 0; --i) {
      double s = (i == t) ? 1.0 : 0.0;
      for (int j = i + 1; j <= t; ++j) s -= R[i][j] * Ri[j][t];
      Ri[i][t] = s / R[i][i];
    }
  }
  __syncthreads();
  for (int i = 0; i < 64; ++i) {
    double v = (i < n && t < n) ? Ri[i][t] : 0.0;
    if (t < n && dead[t]) v = 0.0;
    N[i * 64 + t] = v;
  }
}

__global__ void unblock_basis_kernel(const float* __restrict__ ubt, long D, int K, float* __restrict__ basis, int rp) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= D) return;
  const long blk = c / BG_BLK;
  const int q = (int)(c - blk * BG_BLK);
  for (int k = 0; k < K; ++k) basis[c * K + k] = ubt[blk * rp * BG_BLK + (long)k * BG_BLK + q];
}

struct bg_plan {
  int nblk, rp;
  long ld;
  float *omT, *ypart, *yt, *qt, *bpart, *bm;
  double* gsum;
  tile_la la;   // la.gpart = the Gram matrices of the nblk blocks; one shared mixing matrix
  size_t zero_bytes;
};

// rp = 64 rows of every [comp][x] array while K + 10 <= 64, pmd_tile_rpad(K) beyond (wide.hip kernels)
static void plan_bg(pmd_arena& ar, bg_plan& p, long D, int n, int K) {
  p.nblk = (int)((D + BG_BLK - 1) / BG_BLK);
  p.ld = pmd_time_ld(n);
  p.rp = pmd_tile_rpad(K);
  const size_t nb = p.nblk, rp = p.rp;
  const bool wide = p.rp > 64;
  p.omT = ar.take_n<float>(rp * p.ld);
  p.ypart = wide ? nullptr : ar.take_n<float>(nb * XBT_SLICES * 64 * BG_BLK);   // (the wide path forms Y in one slice)
  p.yt = ar.take_n<float>(nb * rp * BG_BLK);
  p.qt = ar.take_n<float>(nb * rp * BG_BLK);
  p.zero_bytes = ar.used;
  p.bpart = ar.take_n<float>(nb * rp * p.ld);
  p.bm = ar.take_n<float>(rp * p.ld);
  p.la.ctx = nullptr;
  p.la.rp = p.rp;
  p.la.gpart = ar.take_n<double>(nb * rp * rp);
  p.gsum = ar.take_n<double>(rp * rp);
  p.la.nmat = ar.take_n<double>(rp * rp);
  p.la.lam = ar.take_n<double>(rp);
  p.la.eig_ws = nullptr;
  p.la.eig_ws_bytes = 0;
  if (wide) {
    p.la.eig_ws_bytes = pmd_wide_eig_workspace_bytes(p.rp, 1);
    p.la.eig_ws = ar.take(p.la.eig_ws_bytes);
  }
}

extern "C" size_t pmd_background_rsvd_workspace_bytes(long D, int n, int K) {
  pmd_arena ar((void*)0x1000, ~size_t(0) >> 1);
  bg_plan p;
  plan_bg(ar, p, D, n, K);
  return ar.used + 4096;
}

// xs: standardised sample, pixel-major [c][f], leading dimension ld >= pmd_time_ld(n), with the rows of the header's
// contract: round_up(D, 1024) allocated, rows >= D zero (the blocks walked here are BG_BLK = 256 rows, which that covers).
// basis_out: [c][k], K columns.
extern "C" int pmd_background_rsvd(pmd_ctx* ctx, const float* xs, long D, int n, long ld, int K, uint64_t seed,
                                   float* basis_out, void* ws, size_t ws_bytes) {
  CTX_CHECK(ctx);
  const int l = K + 10;
  if (K < 1 || l > 1024) return pmd_fail(ctx, PMD_ERR_UNSUPPORTED, "pmd_background_rsvd", "background_rank must be in [1, 1014]");
  if (ld < pmd_time_ld(n)) return pmd_fail(ctx, PMD_ERR_ARG, "pmd_background_rsvd", "leading dimension too small");
  pmd_arena ar(ws, ws_bytes);
  bg_plan p;
  plan_bg(ar, p, D, n, K);
  if (ar.overflow) return pmd_fail(ctx, PMD_ERR_WORKSPACE, "pmd_background_rsvd", "workspace too small");
  tile_la& la = p.la;
  la.ctx = ctx;
  const int rp = p.rp, nblk = p.nblk;
  const long srb = (long)rp * BG_BLK, srn = (long)rp * p.ld, rp2 = (long)rp * rp;
  PMD_HIP(ctx, hipMemsetAsync(ws, 0, p.zero_bytes, ctx->stream));
  RUN(pmd_launch_rng(ctx, seed, PMD_STREAM_BG_OMEGA, 0, 0, 1, n, l, 1, p.omT, p.ld, 0));
  // Y = X Omega, block by block (Y^T blocks)
  if (la.wide()) {
    RUN(pmd_launch_tile_xbt_rp(ctx, xs, ld, nullptr, 0, BG_BLK, BG_BLK, p.omT, 0, p.ld, p.yt, srb, 0, BG_BLK, nblk, n, 1, l));
  } else {
    RUN(pmd_launch_tile_xbt_rp(ctx, xs, ld, nullptr, 0, BG_BLK, BG_BLK, p.omT, 0, p.ld, p.ypart, XBT_SLICES * srb, srb, BG_BLK, nblk, n, XBT_SLICES, l));
    RUN(pmd_launch_reduce_slices(ctx, p.ypart, XBT_SLICES * srb, srb, XBT_SLICES, srb, p.yt, srb, nblk));
  }
  // tall-skinny orthonormalisation: two rounds of (block Gram matrices, summed) -> whitening -> row mixing.  64 rows:
  // CholeskyQR2 (inverse Cholesky factor); wider: eigen-whitening, which spans the same space
  const float* src = p.yt;
  for (int pass = 0; pass < 2; ++pass) {
    RUN(la.gram(src, BG_BLK, BG_BLK, nblk, 1));
    hipLaunchKernelGGL(sum_gram_blocks_kernel, dim3((unsigned)((rp2 + 255) / 256)), dim3(256), 0, ctx->stream, la.gpart, nblk, p.gsum, (int)rp2);
    PMD_LAUNCH_CHECK(ctx, "sum_gram_blocks_kernel");
    if (la.wide()) {
      RUN(pmd_launch_wide_eig(ctx, p.gsum, 1, rp, l, 1, 1e-13, la.nmat, la.lam, 1, la.eig_ws, la.eig_ws_bytes));
    } else {
      hipLaunchKernelGGL(chol_inverse_kernel, dim3(1), dim3(64), 0, ctx->stream, p.gsum, l, 1e-13, la.nmat);
      PMD_LAUNCH_CHECK(ctx, "chol_inverse_kernel");
    }
    RUN(la.rowmix(src, BG_BLK, l, l, p.qt, BG_BLK, BG_BLK, nblk, true));
    src = p.qt;
  }
  // B = Q^T X (sum of block contributions), SVD via Gram
  RUN(pmd_launch_tile_atx_rp(ctx, xs, ld, nullptr, 0, BG_BLK, BG_BLK, p.qt, srb, BG_BLK, p.bpart, srn, p.ld, nblk, n, 1, l));
  RUN(pmd_launch_reduce_slices(ctx, p.bpart, 0, srn, nblk, srn, p.bm, 0, 1));
  RUN(la.gram(p.bm, p.ld, n, 1, 1));
  RUN(la.eig(1, l, 0, 0.0, la.lam, 1));
  // U = Q u[:, :K]
  RUN(la.rowmix(p.qt, BG_BLK, l, K, p.qt, BG_BLK, BG_BLK, nblk, true));
  hipLaunchKernelGGL(unblock_basis_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, ctx->stream, p.qt, D, K, basis_out, rp);
  PMD_LAUNCH_CHECK(ctx, "unblock_basis_kernel");
  return PMD_OK;
}
