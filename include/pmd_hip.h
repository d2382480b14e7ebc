/*
 * libpmd_hip.so -- C ABI of the MI355X (gfx950) blockwise-PMD hot path.
 *
 * The reference (apasarkar/localmd @ 2025-01-31) has no FFI: its hot path is @jit-ed JAX
 * behind plain Python callables.  Each entry point below replaces the jit region(s) cited
 * next to it (paths under /root/reference/localmd/); INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add to bind them.
 *
 * Conventions
 *   - every function returns int32: 0 = OK, negative = error; pmd_last_error(ctx) has the text
 *   - all pointers are DEVICE pointers owned by the caller unless the name ends in _host
 *   - all work is enqueued on the context's HIP stream (the one given to pmd_ctx_create or pmd_ctx_set_stream): own
 *     kernels, memsets and copies, rocBLAS and rocSOLVER through the context's handle, hipBLASLt per call.  Nothing goes to
 *     the null stream, so a caller may order a call behind its own work on that stream and nowhere else.
 *     Functions that must read a result on the host synchronise that stream themselves, once or more: pmd_orthogonalize,
 *     pmd_orthogonalize_factored, pmd_orthogonalize_chol, pmd_chol_inverse, pmd_projected_svd, pmd_projected_svd_factored,
 *     pmd_psvd_finish, pmd_grid_components, pmdk_syevd, pmdk_sy2sb, pmdk_sytrd2, pmd_profile_query, pmd_ctx_sync; pmd_gemm
 *     and pmd_gram_mtgm where they run fp16-piece products (the operands' exponents are read back); any call that grows
 *     library-owned scratch (the eigensolver's, the split products'), pmd_scratch_trim when it frees some, and
 *     pmd_comm_destroy.  Every other entry point only enqueues.
 *   - scratch memory is a caller-provided workspace; *_workspace_bytes() (*_work_floats()) sizes it.  The workspace starts
 *     on a 256-byte boundary (the library aligns offsets inside it, not addresses).  Its contents on entry are irrelevant
 *     and nothing is kept in it between calls, except where an entry point says so (pmd_stats_stream_*, the staged tile
 *     pipeline, the M^T copy of pmd_gram_mtgm).  A NULL or too-small workspace is refused with PMD_ERR_WORKSPACE (-3)
 *     before anything is launched, written or copied: outputs, inputs and the workspace are as they were, and the context
 *     stays usable (pmd_sliding_extremum / pmd_sliding_quantile report it as PMD_ERR_ARG, pmd_grid_components and the two
 *     pmd_*_moments a NULL one, as any NULL pointer; the two correlations take any size from one frame's partials up).
 *     Nothing outside [ws, ws + ws_bytes) is touched, and the result does not depend on how much more than the reported
 *     size is passed.
 *   - one context per (host thread, device); distinct contexts are independent, also when their streams run at the same
 *     time.  A context owns device scratch that it grows on demand; pmd_scratch_trim frees that of the large products, and
 *     neither growing nor trimming changes a result
 *   (tests/test_gpu_abi_conventions.py: exact size, guard bands and contents for every entry point that takes a workspace
 *   but pmd_sliding_extremum, whose own test has them; refusal and untouched outputs for the decomposition's stages, the
 *   consumers' own tests hold theirs; the stream for every way the library reaches the GPU, not for every entry point.)
 *
 * Layouts
 *   movie        Y[t][c]            frames-first, c = i*d2 + j (what the dataset hands over)
 *   pixel-major  X[c][t]            leading dimension ld = pmd_time_ld(T); zero padded
 *   tile pixels  pix[tile][q]       q = il + b1*jl (column-major inside the tile, as the
 *                                   reference's order="F" reshapes), value = FOV pixel c
 *   tile basis   Ut[tile][comp][q]  rp = pmd_tile_rpad(max_components) component rows (64 up to max_components = 54;
 *                                   rows >= rank are zero), row length pmd_tile_dpad(b1*b2)
 *   tile traces  V[tile][comp][t]   rp component rows, leading dimension ldv >= pmd_time_ld(T)
 *   The global-stage entry points (pmd_weight_tiles, pmd_gram_*, pmd_compact_rows, pmd_tiles_project) take blocks of 64
 *   component rows: an array with rp = 64 v rows is handed to them as v "virtual tiles" per tile, [n*v][64][x], same memory.
 */
#ifndef PMD_HIP_H
#define PMD_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pmd_ctx pmd_ctx;

int pmd_version(void);
/* hip_stream: a hipStream_t (0 = the null stream).  The context never owns the stream.
 * The PMD_* route switches (A/B comparators) are read from the environment when a context is
 * created and are fixed for that context; nothing else in the library reads the environment. */
int pmd_ctx_create(int device, void* hip_stream, pmd_ctx** out);
int pmd_ctx_destroy(pmd_ctx* ctx);
int pmd_ctx_set_stream(pmd_ctx* ctx, void* hip_stream);
int pmd_ctx_sync(pmd_ctx* ctx);
const char* pmd_last_error(pmd_ctx* ctx);

/* Measurement: HIP events on the context's stream around every kernel group (bench.py's
 * roofline figures).  pmd_profile_enable(ctx, 1) resets and starts; pmd_profile_query sums the
 * durations of the groups called `name`; pmd_profile_names lists the names seen. */
int pmd_profile_enable(pmd_ctx* ctx, int on);
int pmd_profile_query(pmd_ctx* ctx, const char* name, double* total_ms, int* count);
int pmd_profile_names(pmd_ctx* ctx, char* buf, int cap);

/* padded sizes every caller needs to allocate buffers */
int pmd_tile_dpad(int d);       /* padded pixel count of a d-pixel tile (-1: unsupported)   */
int pmd_tile_rpad(int r);       /* component rows of the per-tile arrays for max_components = r: 64 while r + 10 <= 64
                                   (the MFMA-tiled main path), round_up(r + 10, 64) beyond (generic-width kernels) */
long pmd_time_ld(long t);       /* leading dimension of a time-contiguous row of t frames   */

/* Gaussian matrices (replaces jax.random.normal: decomposition.py:62,:127,:870; pmd_loader.py:56).
 * Logical array (stream, index0 + b*index_step), rows x cols, element e = row*cols + col, is
 * written to out[b*batch_stride + row*ld + col] (transpose=0) or [.. + col*ld + row] (1). */
int pmd_rng_normal(pmd_ctx* ctx, uint64_t seed, uint32_t stream, uint32_t index0, uint32_t index_step, int batch,
                   long rows, int cols, int transpose, float* out, long ld, long batch_stride);

/* A1: per-pixel mean and Welch noise sigma (pmd_loader.py:203-291; preprocessing_utils.py:10-40).  frame_const: frames per
 * Welch chunk (the reference's 1024), any value >= 1; a chunk of fewer than 256 frames enters the mean only.  T, D or
 * frame_const below 1: PMD_ERR_ARG, and a workspace size of 0. */
size_t pmd_stats_workspace_bytes(int T, long D, int frame_const);
int pmd_stats(pmd_ctx* ctx, const float* movie, int T, long D, int frame_const, int compute_normalizer,
              float* mean_out, float* std_out, void* ws, size_t ws_bytes);

/* (Y - mean)/std of selected frames, transposed to pixel-major (pmd_loader.py:293-298, :376-377,
 * :396-397).  frames: device int32[nf] or NULL for frames 0..nf-1.  out: D rows x ld. */
int pmd_standardize_transpose(pmd_ctx* ctx, const float* movie, long D, const int* frames, int nf, const float* mean,
                              const float* std, float* out, long ld);

/* Streamed ingestion (pmd_loader.py:71-108 FrameDataloader batches, :203-291 statistics pass, :316-346 projection pass):
 * a movie longer than device memory is read in frames-first batches.  Element type of a batch: */
enum pmd_elem { PMD_ELEM_F32 = 0, PMD_ELEM_U16 = 1, PMD_ELEM_I16 = 2 };
#define PMD_STATS_CHUNK 1024   /* frames per Welch chunk of the streamed statistics (frame_const of pmd_stats) */
/* Statistics of a T-frame movie from batches: accumulate frames [t0, t0 + nb) (t0 a multiple of PMD_STATS_CHUNK, nb a
 * multiple of it unless the batch ends the movie) into a workspace that persists over the calls, then finish.  Every
 * chunk must be accumulated once before finish.  fp32 batches give pmd_stats(frame_const = 1024) bit for bit;
 * integer batches give pmd_stats on the fp32-converted movie bit for bit. */
size_t pmd_stats_stream_workspace_bytes(int T, long D);
int pmd_stats_stream_accumulate(pmd_ctx* ctx, const void* batch, int elem, int t0, int nb, int T, long D,
                                int compute_normalizer, void* ws, size_t ws_bytes);
int pmd_stats_stream_finish(pmd_ctx* ctx, int T, long D, int compute_normalizer, float* mean_out, float* std_out,
                            void* ws, size_t ws_bytes);
/* pmd_standardize_transpose on a batch of element type elem (converted to fp32 before (y - mean) / std). */
int pmd_standardize_transpose_typed(pmd_ctx* ctx, const void* movie, int elem, long D, const int* frames, int nf,
                                    const float* mean, const float* std, float* out, long ld);
/* dst[dst_rows[i]] = src[src_rows[i]] for i < n: frames-first rows of D elements of type elem (device index lists). */
int pmd_gather_frames(pmd_ctx* ctx, const void* src, int elem, long D, const int* src_rows, const int* dst_rows, int n,
                      void* dst);

/* Projection of raw frames on a stored spatial basis (pmd_loader.py:316-346, :393-414; localmd_amd/projection.py):
 * Z[row][f] = sum_q A_g[row][q] * (Y[f][pix[pix_off + q]] - mean) / std for every group g and row < r_g, frames f < n
 * of the frames-first batch Y (n x D, element type elem; converted to fp32 before (y - mean) / std).
 * groups: device int64[n_groups][6] = {pix_off, p_g, a_off, out_row, r_g, to_ws}; pix: C-order pixel ids < D;
 * A_g: round_up(r_g, 16) rows x round_up(p_g, 64) fp32 at A + a_off, row-major, zero padded.  to_ws = 0: the group
 * writes rows out_row + row of Z (ld ldz >= n); 1: rows of the partial-sum workspace (n_partial_rows x n fp32), which
 * the call then reduces: wide: device int64[n_wide_rows][4] = {z_row, ws_row0, parts, stride},
 * Z[z_row][f] = sum_{c < parts} ws[ws_row0 + c stride][f] in order c = 0, 1, ...  The tables are trusted (the caller
 * validates them); rows of Z outside every group are not written.  No synchronisation, no allocation. */
size_t pmd_group_project_workspace_bytes(long n_partial_rows, int n);
int pmd_group_project(pmd_ctx* ctx, const void* Y, int elem, int n, long D, const float* mean, const float* std,
                      int n_groups, const long* groups, const int* pix, const float* A, long n_partial_rows,
                      int n_wide_rows, const long* wide, float* Z, long ldz, void* ws, size_t ws_bytes);

/* Fused expansion of a decomposition into output frames (localmd_amd/export.py): for the n frames of one call,
 *   x[f][c] = mean[c] + std[c] * sum_e sum_{k < r_e} A[a_off_e + k p64_e + qmap[64 e + c mod 64]] * C[c_row0_e + k][f]
 * over the entries e of patch c / 64 (patch_ptr[patch] <= e < patch_ptr[patch + 1], n_patches = ceil(d1 d2 / 64)),
 * entries: device int64[n_entries][4] = {a_off, p64, r (1..64), c_row0}; qmap: int32[n_entries][64] with -1 for a
 * pixel outside the entry's group; A: the group blocks of pmd_group_project (rows padded to 16).  C: rows x ldc fp32,
 * column f = frame f of the call.  Y: the raw frames-first batch (element type y_elem, ldy >= d1 d2 elements per frame,
 * frame f of the call at Y + f ldy), read only when a panel needs it.  Panel p (< n_panels <= 3) is
 * (panels >> 2p) & 3: 0 raw y, 1 denoised x, 2 residual y - x (from the rounded x); out (element type out_elem,
 * frame f at out + f d1 n_panels d2 elements) gets out[f][i][p d2 + j] for pixel c = i d2 + j.  Integer outputs round
 * half to even and saturate, NaN -> 0.  The tables are trusted (the caller validates them).  Frame f's bits do not
 * depend on n or on the call it comes in.  No synchronisation, no allocation, no workspace. */
int pmd_group_expand(pmd_ctx* ctx, const float* C, long ldc, int n, int d1, int d2, const float* mean, const float* std,
                     long n_patches, const long* patch_ptr, long n_entries, const long* entries, const int* qmap,
                     const float* A, const void* Y, int y_elem, long ldy, int n_panels, int panels, void* out,
                     int out_elem);

/* ROI traces (localmd_amd/traces.py).  pmd_roi_gather: out[k][f] = sum_q w[q] * (float) Y[f][pix[q]] over the pixels of
 * ROI k, for the n frames of a frames-first batch Y (n x D, element type elem, converted to fp32 in the kernel).
 * pix / w: the C-order pixel ids (< D, ascending within an ROI) and weights of all ROIs, one after the other.
 * segs: device int64[n_segs][4] = {q0, p (>= 1), out_row, to_ws}: p pixels from pix + q0; to_ws = 0: the segment is a
 * whole ROI and writes row out_row of out (ld ldo >= n); 1: it is one piece of a split ROI and writes row out_row of
 * the partial-sum workspace (n_partial_rows x n fp32), which the call then reduces: split: device
 * int64[n_split][3] = {out_row, ws_row0, parts}, out[out_row][f] = sum_{c < parts} ws[ws_row0 + c][f], c = 0, 1, ...
 * Sum of a segment: lane l (of 64) runs one fma chain over its pixels l, l + 64, ... from 0, then an xor butterfly
 * (1, 2, ..., 32) folds the lanes; the order depends on the tables alone, so out[k][f] has the same bits for every n,
 * every position of the frame in its batch and every element type holding the same values.  The tables are trusted
 * (the caller validates them: traces.validate_roi_tables); rows of out that no segment / split entry names are not
 * written.  No atomics, no synchronisation, no allocation.
 * pmd_roi_combine: d = C[k][f] + offset[k] (C == NULL: d = offset[k]) for k < K, f < n; den[k][f] = d (den may be
 * NULL); res[k][f] = raw[k][f] - d, from the rounded d (res may be NULL; raw is read only for res). */
size_t pmd_roi_gather_workspace_bytes(long n_partial_rows, int n);
int pmd_roi_gather(pmd_ctx* ctx, const void* Y, int elem, int n, long D, long n_segs, const long* segs, const int* pix,
                   const float* w, long n_partial_rows, int n_split, const long* split, float* out, long ldo, void* ws,
                   size_t ws_bytes);
int pmd_roi_combine(pmd_ctx* ctx, long K, int n, const float* C, long ldc, const float* offset, const float* raw, long ldr,
                    float* den, long ldd, float* res, long lde);

/* Per-pixel regressor maps (localmd_amd/maps.py): one block of n frames of a batch against K time courses. */
#define PMD_REGRESS_BLOCK 1024
/* acc[k][c] += sum_{f < n} X[k][f] * z[f][c]   for k < K, c < D,   z[f][c] = (float) Y[f][c] - mean[c]  (mean NULL: no shift)
 * mom[c] += sum_f z[f][c],  mom[D + c] += sum_f z[f][c]^2          (mom NULL: not formed; K = 0 with mom is allowed)
 * Y: frames-first batch, element type elem, frame f at Y + f ldy elements (ldy >= D); X: K rows, ld ldx >= n, column f =
 * frame f of the call; n <= PMD_REGRESS_BLOCK.  Every sum of the call is formed in fp32 in an order fixed by n alone,
 * converted to double and added to acc / mom once; one owner per element: no atomics.  The bits a call adds to acc[k][c]
 * depend on row k of X, column c of Y and mean[c] only: not on K, on the other rows, on ldy / ldx / lda, nor on the element
 * type holding the same values.  No synchronisation, no allocation, no workspace. */
int pmd_regress_accumulate(pmd_ctx* ctx, const void* Y, int elem, long ldy, int n, long D, const float* mean,
                           const float* X, long ldx, int K, double* acc, long lda, double* mom);

/* Per-pixel summary images (localmd_amd/summary.py): extrema and power sums of one block of n frames of a batch. */
#define PMD_STATS_BLOCK 1024
/* Y: frames-first batch, element type elem (converted to fp32 exactly), frame f of the call at Y + f ldy elements
 * (ldy >= D); 1 <= n <= PMD_STATS_BLOCK; f0: the frame number of the call's first frame, a multiple of bin, f0 + n < 2^31;
 * bin: a power of two <= PMD_STATS_BLOCK.  The call's frames are taken in four slices of 256, slice w = frames
 * [256 w, min(n, 256 w + 256)); a slice from n on is empty.
 * ext != NULL (ext[c] the minimum, ext[D + c] the maximum; arg, which may be NULL, the frame numbers in the same layout):
 *   bin == 1: the value of frame f is (float) Y[f][c], no arithmetic.  Otherwise the values are those of the bins
 *   [b, min(n, b + bin)), b a multiple of bin: the fp32 sum of the bin's frames divided (IEEE) by their count.  The sum of
 *   a bin <= 256 is one chain over its frames in ascending order, starting from the first frame's value; for bin = 512
 *   and 1024 every slice of the bin is summed so and the slice sums are added in ascending slice order, starting from the
 *   first.  A value v replaces ext[c] only if v < ext[c] and ext[D + c] only if v > ext[D + c], values in ascending frame
 *   order, and arg gets f0 + (first frame of the bin): the first frame that attains an extremum keeps arg, within a call
 *   and across calls in frame order; a NaN value never becomes an extremum.
 * mom != NULL: z = fl((float) Y[f][c] - centre[c]) (centre NULL: no shift), mom[p D + c] += sum_f z^(p + 1), p = 0 .. 3,
 *   the powers as z2 = fl(z z), fl(z2 z), fl(z2 z2).  Each sum is formed in fp32: one chain per slice over its frames in
 *   ascending order from 0, the slice sums added in ascending slice order; then converted to double and added once.
 * One owner per pixel: no atomics.  The bits written for pixel c depend on column c of Y, centre[c], n, f0, bin and the
 * previous state only: not on D, ldy, the element type holding the same values, the pixel's position, or on which of
 * ext / arg / mom the call forms.  Errors (nothing is launched): n out of range, bin not a power of two or too large, f0
 * not a multiple of bin, ext and mom both NULL, arg without ext, unknown elem, ldy < D.  No synchronisation, no
 * allocation, no workspace. */
int pmd_pixel_stats_accumulate(pmd_ctx* ctx, const void* Y, int elem, long ldy, int n, long D, long f0, int bin,
                               const float* centre, float* ext, int* arg, double* mom);

/* Exact per-pixel order statistics over time (localmd_amd/quantiles.py): a radix select over per-pixel histograms, most
 * significant 8-bit digit first.  Key of element y of pixel c: v = (float) Y[f][c]; centre != NULL: v = |v - centre[c]|
 * (one fp32 subtraction, round to nearest, no contraction; denormal differences are kept, not flushed).  key = ~bits(v)
 * when the sign bit of v is set, bits(v) | 0x80000000 otherwise, 0xFFFFFFFF for every NaN: keys order as the values do,
 * -0 before +0 and NaN last.
 * hist: uint32 [ceil(D / 64)][256][64] indexed (pixel group, bin, pixel in group), 16-byte aligned, zero before the first
 * call of a pass.
 * pmd_pixel_hist_accumulate: for the n >= 1 frames of a frames-first batch (element type elem, frame f at Y + f ldy
 * elements, ldy >= D; any n < 2^31, no block discipline: counting is order-free) element (f, c) is counted when pass == 0
 * or key >> (32 - 8 pass) == prefix[c], in bin (key >> (24 - 8 pass)) & 255 of pixel c; pass in 0 .. 3, prefix may be NULL
 * for pass 0.  One workgroup owns a pixel group: no global atomics.
 * pmd_pixel_hist_select: per pixel c < D the first bin b whose cumulative count exceeds rank[c] (0 <= rank[c] < the
 * pixel's count); rank[c] -= the count below b, prefix[c] = prefix[c] << 8 | b; a pixel whose rank is not below its count
 * keeps rank and prefix.  Every count of hist is set to zero.  After the last pass prefix[c] is the key of the
 * order statistic.
 * Errors (nothing is launched): n < 1, D < 1, ldy < D, pass outside 0 .. 3, unknown elem, a NULL Y / hist / rank, prefix
 * NULL where it is read, hist not 16-byte aligned.  No synchronisation, no allocation, no workspace. */
int pmd_pixel_hist_accumulate(pmd_ctx* ctx, const void* Y, int elem, long ldy, long n, long D, const float* centre,
                              int pass, const uint32_t* prefix, uint32_t* hist);
int pmd_pixel_hist_select(pmd_ctx* ctx, long D, uint32_t* hist, int* rank, uint32_t* prefix);

/* Rolling baseline and dF/F along time (localmd_amd/baseline.py, csrc/baseline.hip): the series of a pixel is reduced to
 * knots (bin means), the knots are filtered by a sliding minimum and / or maximum or by a sliding order statistic, and the
 * baseline of a frame is
 * interpolated between the knots.  All matrices are frames-first with a leading dimension in elements; every fp32
 * operation below is rounded on its own (no contraction).  The bits written for pixel c depend on column c of the inputs
 * and the scalar arguments only: not on N, the leading dimensions, alignment, the element type holding the same values
 * or the pixel's position.  None of them synchronises or allocates; an argument error returns PMD_ERR_ARG with
 * nothing launched.
 *
 * pmd_bin_means: Y holds the n frames f0 .. f0 + n of a series (1 <= n <= PMD_STATS_BLOCK, element type elem, ldy >= N);
 *   bin is a power of two in 1 .. PMD_BASELINE_MAX_BIN, f0 >= 0 a multiple of it, f0 + n < 2^31.  Bins start at
 *   multiples of bin; the bins [b, min(n, b + bin)) of the call are written to the rows f0 / bin + b / bin of K (fp32,
 *   ldk >= N): the fp32 chain over the bin's frames in ascending order starting from the first frame's value, divided
 *   (IEEE) by the frame count (the call's last bin may be short); bin == 1: (float) Y[f][c], no arithmetic.  The
 *   definition of pmd_pixel_stats_accumulate for bin <= 256.
 *   Errors: n or bin out of range, f0 negative or not a multiple of bin, N < 1, ldy < N, ldk < N, unknown elem, NULL Y / K.
 *
 * pmd_sliding_extremum: out[j][c] = fminf (is_max = 0) or fmaxf (is_max = 1) over X[max(0, j - half) .. min(n - 1,
 *   j + half)][c], for the n >= 1 rows of X (n x N fp32, ldx >= N) into out (n x N, ldo >= N, no overlap with X); half >= 0
 *   may exceed n.  A NaN is dropped unless every frame of the window is NaN; -0 and +0 compare equal and either may come
 *   out.  The work per output does not depend on half (segment prefix / suffix extrema).  work: at least
 *   pmd_sliding_extremum_work_floats(n, N) = n * round_up(N, 4) floats of device memory that overlap neither matrix; a
 *   caller bounds it by calling once per range of Nc columns (X + c0, out + c0, N = Nc, the same leading dimensions).
 *   Errors: n < 1, N < 1, N > 65535 * 256, ldx < N, ldo < N, half < 0, is_max not 0 / 1, a NULL pointer, work_floats too
 *   small, X and out overlapping.
 *
 * pmd_sliding_quantile: the sliding order statistic.  X is n x N fp32, frames-first, ldx >= N; out is n x N, ldo >= N, and
 *   does not overlap X.  W = 2 half + 1.  The window of output (j, c) is the multiset X[clamp(j + i, 0, n - 1)][c] for
 *   i = -half .. half: the edges are replicated (scipy.ndimage's mode "nearest"), not cut, so every window has W members
 *   and one rank serves every output.  out[j][c] is the member at 0-based position rank when the window is ordered by the
 *   keys of pmd_pixel_hist_accumulate (quantiles.float_keys: -0 before +0, every NaN last); the value written is
 *   quantiles.key_floats of that key, so a NaN comes out as the NaN with the bits 0x7FFFFFFF.  rank = 0 is the sliding
 *   minimum that drops NaN unless the whole window is NaN, rank = 2 half the maximum with NaN winning.  half >= 0 may
 *   exceed n.
 *   The bits of column c depend on column c, n, half and rank only: not on N, the leading dimensions, alignment, the
 *   column's position or a split into column ranges (X + c0, out + c0).  No global atomics.  A wave takes
 *   PMD_SLIDING_QUANTILE_SLICE consecutive outputs: a 32-step bisection on the key for the first, then per output one
 *   member leaves and one enters and the answer moves by at most one distinct value, found by one scan of the window.
 *   The element visits per output and column are O(min(W, n)): a scan reads the rows the window really holds once, and
 *   counts the replicated first and last row with a multiplicity.
 *   work: at least pmd_sliding_quantile_work_floats(n, N, half) floats of device memory; the query returns 0 (the state
 *   lives in registers) and work may then be NULL.
 *   Errors: n < 1 or n >= 2^31, N < 1, N > 65535 * 256, ldx < N, ldo < N, half < 0 or half >= 2^30, rank outside
 *   0 .. 2 half, NULL X or out, X and out overlapping, work_floats below the query (or NULL work with a query above 0).
 *
 * pmd_baseline_apply: frames f0 .. f0 + n (1 <= n <= PMD_STATS_BLOCK, f0 >= 0, f0 + n <= T) of a series of T frames,
 *   1 <= T < PMD_BASELINE_MAX_FRAMES, whose ceil(T / bin) knots are the rows of K (ldk >= N).  Bin j has n_j = min(bin,
 *   T - j bin) frames and the centre c_j = j bin + (n_j - 1) / 2 (exact in fp32).  The baseline F0 of frame t: K_0 for
 *   t <= c_0, K_last for t >= c_last; else with j the last bin with c_j <= t: K_j when t == c_j (no arithmetic), otherwise
 *   w = (t - c_j) / (c_{j+1} - c_j) (one fp32 division of exact operands), F0 = K_j + w (K_{j+1} - K_j).  With
 *   x = (float) X[t - f0][c]: out (fp32, ldo >= N) gets F0 (mode 0; X may be NULL and is not read), x - F0 (mode 1), or
 *   (x - F0) / F0 where F0 > min_baseline and 0 elsewhere, a NaN F0 included (mode 2).
 *   Errors: n, bin, T or mode out of range, frames outside 0 .. T, N < 1, a leading dimension below N, unknown elem, NULL
 *   K / out, NULL X with mode 1 or 2. */
#define PMD_BASELINE_MAX_BIN 256
#define PMD_BASELINE_MAX_FRAMES (1L << 23)
int pmd_bin_means(pmd_ctx* ctx, const void* Y, int elem, long ldy, int n, long N, long f0, int bin, float* K, long ldk);
long pmd_sliding_extremum_work_floats(long n, long Nc);
int pmd_sliding_extremum(pmd_ctx* ctx, const float* X, long ldx, long n, long N, long half, int is_max, float* out,
                         long ldo, float* work, long work_floats);
#define PMD_SLIDING_QUANTILE_SLICE 128
long pmd_sliding_quantile_work_floats(long n, long Nc, long half);
int pmd_sliding_quantile(pmd_ctx* ctx, const float* X, long ldx, long n, long N, long half, long rank, float* out,
                         long ldo, float* work, long work_floats);
int pmd_baseline_apply(pmd_ctx* ctx, const void* X, int elem, long ldx, int n, long N, long f0, long T, int bin,
                       const float* K, long ldk, int mode, float min_baseline, float* out, long ldo);

/* Demixing of overlapping ROIs (localmd_amd/demix.py, csrc/hals.hip): the two non-negative Gauss-Seidel (HALS) sweeps
 * of x ~ A c + b.  Every fp32 operation is rounded on its own (no contraction), in the order written here.  Neither
 * synchronises or allocates; an argument error returns PMD_ERR_ARG with nothing launched.
 *
 * pmd_hals_sweep: over the columns t < n of C (K rows, ldc >= n; updated in place) with P (K rows, ldp >= n) and the CSR
 *   matrix G = (indptr[K + 1], indices, data) whose rows hold their diagonal entry.  For every t, and for k = 0 .. K - 1
 *   in order: acc = P[k][t]; for the nonzeros i of row k in stored order acc = acc - data[i] * C[indices[i]][t] (the
 *   newest values: rows below k are those of this sweep); C[k][t] = max(lo[k], C[k][t] + acc * invd[k]), with invd[k] =
 *   1 / G[k][k] and lo[k] = 0 or -inf.  A row with invd[k] == 0 is not touched, nor is anything beyond column n.  The
 *   bits of column t depend on column t alone: a call may be split into column ranges.  n == 0 does nothing.
 *   Errors: K < 1, n < 0, ldc < n, ldp < n, a NULL pointer.
 *
 * pmd_hals_pixels: over n_px pixels.  Pixel q is row px_row[q] of the CSR matrix U = (u_indptr, u_indices, u_data) and
 *   is covered by the pairs j in [cov_ptr[q], cov_ptr[q + 1]), at most PMD_HALS_MAX_COVER of them, of ROI cov_k[j] and
 *   footprint value a[j].  Sy_j = scale[q] * sum_i u_data[i] * Mt[cov_k[j]][u_indices[i]] over the nonzeros of the row
 *   (Mt: K rows, ld ldm), then for the pairs in ascending j, each reading the newest values,
 *   a[j] = max(0, a[j] + (Sy_j - sum_j' a[j'] H[cov_k[j']][cov_k[j]]) / H[cov_k[j]][cov_k[j]]) (H: K x K, ld ldh).  A
 *   pair whose H[k][k] == 0 or frozen[k] != 0 is not written.  The tables are trusted (the caller validates them); a
 *   pixel with more than PMD_HALS_MAX_COVER pairs is skipped.  Errors: n_px < 0, a NULL pointer. */
#define PMD_HALS_MAX_COVER 64
int pmd_hals_sweep(pmd_ctx* ctx, float* C, long ldc, const float* P, long ldp, int K, long n, const int64_t* indptr,
                   const int* indices, const float* data, const float* invd, const float* lo);
int pmd_hals_pixels(pmd_ctx* ctx, long n_px, const int* px_row, const int64_t* cov_ptr, const int* cov_k, float* a,
                    const int64_t* u_indptr, const int* u_indices, const float* u_data, const float* scale,
                    const float* Mt, long ldm, const float* H, long ldh, const int* frozen);

/* Superpixel seeds (localmd_amd/superpixels.py, csrc/superpixel.hip): the neighbour moments of the thresholded movie and
 * the connected components of a per-edge pixel graph.  Images are d1 x d2 in natural orientation, pixel c = i d2 + j.
 *
 * pmd_threshold_moments_accumulate: Y is a frames-first batch of element type elem (converted to fp32 exactly), frame f
 *   of the call at Y + f ldy elements, ldy >= D = d1 d2; any n >= 1 (no block discipline).  With v = (float) Y[f][c]:
 *   y = v > thr[c] ? fl32(v - thr[c]) : 0, so a NaN value or a NaN threshold gives 0.  mom is double [6][D] and is added
 *   to: mom[0] += sum_f y, mom[1] += sum_f y^2, mom[2 .. 5] += sum_f y_p y_q for the forward neighbours q of p in the
 *   order E (0, +1), SW (+1, -1), S (+1, 0), SE (+1, +1); a neighbour outside the image contributes 0.  Every product is
 *   formed in fp64 from the fp32 y and is exact; every sum is one fp64 chain per pixel over the frames in ascending
 *   order, continued from the stored value.  The bits of pixel c therefore depend on the columns of c and of its forward
 *   neighbours, their thresholds and the previous state only: not on how the frames are split over calls, on ldy, on the
 *   element type holding the same values, nor on the pixel's position.  One owner per pixel: no atomics, no workspace,
 *   no synchronisation, no allocation.
 *   Errors (PMD_ERR_ARG, nothing is launched): n < 1, d1 < 1, d2 < 1, ldy < D, unknown elem, a NULL pointer, more than
 *   65535 * 62 columns.
 *
 * pmd_grid_components: edges[c] is one byte, bit 0: c is joined to its E neighbour, bit 1: SW, bit 2: S, bit 3: SE; a
 *   bit that points outside the image and the high four bits are ignored.  label[c] (int32) becomes the smallest pixel
 *   index of the connected component of c; an isolated pixel is its own root.  The result is fully determined by the
 *   input.  Three launches (tiles in LDS, the tile borders on label, flattening); every cross-workgroup access to label
 *   is a relaxed agent-scope atomic, parents are only ever lowered, and no workgroup waits for another.  ws: at least
 *   pmd_grid_components_workspace_bytes bytes of device memory (a give-up flag, cleared by every call).  The call
 *   synchronises the stream once, to read that flag: should a union reach its round limit (2 D + 2, which the algorithm
 *   cannot reach) it returns PMD_ERR_UNSUPPORTED and label is not valid.  No allocation.
 *   Errors (nothing is launched): d1 < 1, d2 < 1, d1 d2 >= 2^31, a NULL pointer (PMD_ERR_ARG); ws_bytes too small
 *   (PMD_ERR_WORKSPACE). */
int pmd_threshold_moments_accumulate(pmd_ctx* ctx, const void* Y, int elem, long ldy, int n, int d1, int d2,
                                     const float* thr, double* mom);
size_t pmd_grid_components_workspace_bytes(int d1, int d2);
int pmd_grid_components(pmd_ctx* ctx, int d1, int d2, const uint8_t* edges, int* label, void* ws, size_t ws_bytes);

/* Growing ROI supports (localmd_amd/grow.py, csrc/roigrow.hip): per (pixel, ROI) pair of every ROI's window, the moments
 * of the movie, with the other ROIs of that pixel taken out, against the ROI's trace.
 *
 * pmd_roi_window_moments_accumulate: X is a frames-first batch of element type elem (converted to fp32 exactly), frame f
 *   of the call at X + f ldx elements, ldx >= D; any n >= 1 (no block discipline).  Ct holds the traces frames-first: the
 *   K values of frame f at Ct + f ldct, ldct >= K.  Pair i < n_pairs is pixel pair_px[i] (0 <= pair_px[i] < D) and ROI
 *   pair_k[i] (0 <= pair_k[i] < K); its others are the entries q in [oth_ptr[i], oth_ptr[i + 1]), ROI oth_k[q] with the
 *   footprint value oth_a[q] on that pixel, any number of them (demix allows PMD_HALS_MAX_COVER ROIs on a pixel).  Per
 *   pair and frame, every fp32 operation rounded on its own (no contraction), in this order: y = (float) X[f][pair_px[i]];
 *   for q in stored order y = fl32(y - fl32(oth_a[q] * Ct[f][oth_k[q]])); c = Ct[f][pair_k[i]].  mom is double
 *   [3][n_pairs] and is added to: mom[0][i] += sum_f y, mom[1][i] += sum_f y^2, mom[2][i] += sum_f y c.  Both products are
 *   formed in fp64 from fp32 values and are exact; every sum is one fp64 chain per pair over the frames in ascending
 *   order, continued from the stored value.  The bits of pair i therefore depend on its pixel's column, the trace rows
 *   it names, its oth_a and the previous state only: not on how the frames are split over calls, on ldx or ldct, on the
 *   element type holding the same values, on the pair's position in the table, nor on what other pairs are present.  The
 *   tables are trusted (the caller validates them).  One owner per pair: no atomics, no workspace, no synchronisation, no
 *   allocation.  n_pairs == 0 does nothing.
 *   Errors (PMD_ERR_ARG, nothing is launched, mom untouched): n < 1, K < 1, D < 1, ldx < D, ldct < K, n_pairs < 0,
 *   unknown elem, a NULL pointer with n_pairs > 0, more than (2^31 - 1) * 256 pairs. */
int pmd_roi_window_moments_accumulate(pmd_ctx* ctx, const void* X, int elem, long ldx, long D, int n, const float* Ct,
                                      long ldct, int K, long n_pairs, const int* pair_px, const int* pair_k,
                                      const int64_t* oth_ptr, const int* oth_k, const float* oth_a, double* mom);

/* Spike inference (localmd_amd/deconvolve.py, csrc/oasis.hip): OASIS for an AR(1) model, n_prob independent problems in
 * one launch.  Y is frames-first (frame t at Y + t ldy elements); problem p reads column col[p] (0 <= col[p] < ldy), its
 * parameters par[4 p .. 4 p + 3] = g, lam, s_min, b, and the table row pw + pw_row[p] ldpw, whose entry l = 0 .. T is g^l
 * rounded to fp32 (built by the caller; the kernel never forms a power, it only indexes the row).  It minimises
 * 1/2 |c + b - y|^2 + lam sum_t s_t over s_t = c_t - g c_{t-1} >= 0 (s_min > 0: the hard-threshold variant) by
 * pool-adjacent-violators.  Every fp32 operation below is rounded on its own (no contraction), divisions are IEEE,
 * denormals are kept:
 *   forward, t = 0 .. T - 1: mu = lam * (1 - g); y' = (y[t] - b) - (t < T - 1 ? mu : lam); push the pool (v, w, t0, l) =
 *     (y', 1, t, 1); while there are >= 2 pools and v_i < v_{i-1} * pw[l_{i-1}] + s_min, with q = pw[l_{i-1}]:
 *     num = w_{i-1} * v_{i-1} + (q * w_i) * v_i; den = w_{i-1} + (q * q) * w_i; v_{i-1} = num / den; w_{i-1} = den;
 *     l_{i-1} += l_i; pop.  den >= 1.  A NaN never compares true and never merges.
 *   fill, pool k: vp = v_k > 0 ? v_k : 0; c[t0_k + j] = vp * pw[j] for j < l_k; s = 0 except at the first frame of a
 *     pool k >= 1, where with d = c[t0_k] - g * c[t0_k - 1], s[t0_k] = d > 0 ? d : 0.
 *   residual: d_t = y[t] - (c[t] + b); rss = sum_t (double) d_t * (double) d_t, one fp64 chain in ascending t.
 * C and S (T rows of n_prob columns, ldc, lds >= n_prob), rss[n_prob] and n_pools[n_prob] (the number of pools at the
 * end) may each be NULL.  The bits of a problem depend on its column, its four parameters and its table row only: not
 * on n_prob, its position, the leading dimensions, which outputs are requested, or how problems are split over calls.
 * col and pw_row are trusted (the caller validates them).  ws: pmd_oasis_ar1_workspace_bytes(T, n_prob) =
 * 12 T n_prob bytes (the pool stacks).  No synchronisation, no allocation.
 * Errors (nothing is launched): T < 1, T >= 2^31 - 1, n_prob < 1, ldy < 1, ldpw < T + 1, ldc or lds < n_prob, a NULL
 * Y / col / par / pw_row / pw, all four outputs NULL (PMD_ERR_ARG); ws NULL or too small (PMD_ERR_WORKSPACE). */
size_t pmd_oasis_ar1_workspace_bytes(long T, long n_prob);
int pmd_oasis_ar1(pmd_ctx* ctx, const float* Y, long ldy, long T, long n_prob, const int* col, const float* par,
                  const int* pw_row, const float* pw, long ldpw, float* C, long ldc, float* S, long lds, double* rss,
                  int* n_pools, void* ws, size_t ws_bytes);

/* Spike inference for an AR(2) model with a finite rise time (deconvolve(p=2), csrc/oasis2.hip): the greedy pooled solver
 * of Friedrich, Zhou & Paninski 2017, Alg. 3, with O(1) merges.  Arguments and conventions are those of pmd_oasis_ar1
 * except: par[5 p .. 5 p + 4] = g1, g2, lam, s_min, b (admissible: the roots 0 <= r <= d < 1 of z^2 - g1 z - g2 are real,
 * so g1 >= 0, g2 <= 0; trusted), and tab_row[p] selects three consecutive rows of tab (ldtab >= T + 2 apart), built by the
 * caller (deconvolve.ar2_tables): H[i] = h_{i-1}, i = 0 .. T + 1, with h_{-1} = 0, h_0 = 1, h_j = g1 h_{j-1} + g2 h_{j-2};
 * HH[l] = sum_{j<l} h_j^2 and HK[l] = sum_{j<l} h_j h_{j-1}, l = 0 .. T.  The kernel only indexes them.  It minimises
 * 1/2 |c + b - y|^2 + lam sum_t s_t over s_t = c_t - g1 c_{t-1} - g2 c_{t-2} >= 0 (c_{-1} = c_{-2} = 0, s_0 = c_0 >= 0
 * free), greedily: the value under a pool is held fixed while the pool is refitted, so for g2 != 0 the result is close
 * to the optimum, not the optimum.  Every fp32 operation below is rounded on its own (no contraction; each product and
 * each sum written here is one operation, evaluated left to right inside its brackets), divisions are IEEE, denormals
 * are kept.  A pool is (v, w, N, M, t0, l); gw of a pool is g2 * w of the pool underneath, g2 * 0 for the bottom pool.
 *   penalties: mu = lam * ((1 - g1) - g2), mu1 = lam * (1 - g1); pen_t = mu for t < T - 2, mu1 for t = T - 2, lam for
 *     t = T - 1; y' = (y[t] - b) - pen_t.
 *   forward, t = 0 .. T - 1: push (v, w, N, M, t0, l) = (y', y', y', 0, t, 1); when it is the bottom pool, v and w are
 *     (y' > 0 ? y' : 0) and N stays y'.  While there are >= 2 pools, with k the pool under the top, m = l_k:
 *     pred = H[m+1] * v_k + H[m] * gw_k; if not v_top < pred + s_min, stop.  Merge: gm = g2 * M_top;
 *     N_k = N_k + (H[m+1] * N_top + H[m] * gm); M_k = M_k + (H[m] * N_top + H[m-1] * gm); l_k += l_top; pop; set pool k
 *     with l = l_k: v_k = (N_k - gw_k * HK[l]) / HH[l]; the bottom pool alone: v_k = v_k > 0 ? v_k : 0;
 *     w_k = H[l] * v_k + H[l-1] * gw_k.  HH[l] >= 1.  A NaN never compares true and never merges; every iteration pops
 *     a pool, so the loop ends on any input.
 *   fill, pool k: c[t0_k + j] = H[j+1] * v_k + H[j] * gw_k for j < l_k; s = 0 except at the first frame t of a pool
 *     k >= 1, where d = c[t] - g1 * c[t-1], then for t >= 2 d = d - g2 * c[t-2], and s[t] = d > 0 ? d : 0.
 *   residual: as pmd_oasis_ar1.  n_pools is the final depth.
 * The bits of a problem depend on its column, its five parameters and its three table rows only.
 * ws: 24 T n_prob bytes, which is pmd_oasis_ar1_workspace_bytes(T, 2 n_prob): five words per pool and one spare.
 * Errors (nothing is launched): as pmd_oasis_ar1, with ldtab < T + 2 in the place of ldpw < T + 1. */
int pmd_oasis_ar2(pmd_ctx* ctx, const float* Y, long ldy, long T, long n_prob, const int* col, const float* par,
                  const int* tab_row, const float* tab, long ldtab, float* C, long ldc, float* S, long lds, double* rss,
                  int* n_pools, void* ws, size_t ws_bytes);

/* Rigid motion correction by template matching (localmd_amd/register.py, csrc/register.hip).  A frame is d1 x d2; the
 * window is rows [my, d1 - my) x columns [mx, d2 - mx) of the template, h x w pixels, h, w >= PMD_SHIFT_MIN_WINDOW.
 * tp is the fp32 template on the window minus its mean, row-major h x w.  With sy = dy + my, sx = dx + mx the surface of
 * frame f is C[sy][sx] = sum_{i < h, j < w} tp[i][j] f[i + sy][j + sx] for 0 <= sy <= 2 my, 0 <= sx <= 2 mx: the
 * un-normalised zero-mean cross-correlation; every term lies inside the frame and every shift sums h w terms.
 *
 * The correlation: n frames of element type elem (widened in registers), frame k at X + k frame_stride elements, the
 *   image's pixel (y, x) at (y0 + y) row_stride + x0 + x inside it.  surf receives n (2 my + 1)(2 mx + 1) floats.
 *   The window is cut into tiles of 32 rows x 64 columns; a tile's sum is an fmaf chain over its rows (in S = 4, 2 or 1
 *   row ranges for (2 my + 1) ceil((2 mx + 1) / 8) <= 64, <= 128, above; the ranges are added in ascending order) and
 *   columns in ascending order, and the tiles are added in ascending (row-major) order.  No atomics: the bits of a frame
 *   depend on the frame, tp and the geometry only.  ws holds the tile partials of a launch group; the workspace function
 *   sizes it for min(n, 64 MB worth of) frames, and any size of at least one frame's partials
 *   (4 tiles (2 my + 1)(2 mx + 1) bytes) is taken.  Errors: n < 0, my or mx outside 1 .. PMD_SHIFT_MAX, d1 or d2 above
 *   PMD_SHIFT_MAX_DIM, a window below 8 x 8, an unknown elem, y0 or x0 < 0, row_stride < x0 + d2, frame_stride <
 *   (y0 + d1 - 1) row_stride + x0 + d2, a NULL X / tp / surf (PMD_ERR_ARG); ws NULL or too small (PMD_ERR_WORKSPACE).
 * The peak: per frame arg = (dy, dx) of the first maximum of the surface in row-major order, NaN entries skipped;
 *   peak its value; neigh the 3 x 3 entries around it (row-major, NaN outside the surface).  A surface without a finite
 *   entry gives (0, 0), NaN and nine NaN.
 * The shifted movie: out[k][y][x] from frame k shifted by ishift[2 k], ishift[2 k + 1] (the floors of the shift) and the
 *   bilinear weights wts[4 k .. 4 k + 3] = w00, w01, w10, w11 of the samples a = f[y + iy][x + ix], b = f[y + iy][x + ix + 1],
 *   c = f[y + iy + 1][x + ix], d = f[y + iy + 1][x + ix + 1].  Samples outside the frame are those of the nearest edge
 *   pixel (border PMD_SHIFT_BORDER_NEAREST) or fill (PMD_SHIFT_BORDER_CONSTANT).  A frame with weights exactly
 *   (1, 0, 0, 0) is copied: bit for bit when elem == out_elem, else converted (exactly, or quantised as below).  Every
 *   other frame is fl(fl(fl(w00 a) + fl(w01 b)) + fl(fl(w10 c) + fl(w11 d))), no contraction; 16-bit outputs round half
 *   to even, saturate, NaN -> 0.  Errors: n < 0, sides outside 1 .. PMD_SHIFT_MAX_DIM, unknown elem / out_elem / border,
 *   a stride shorter than a row or a frame, a NULL pointer, X and out overlapping (PMD_ERR_ARG).
 * None of the three synchronises or allocates; n == 0 launches nothing and returns PMD_OK. */
#define PMD_SHIFT_MAX 31
#define PMD_SHIFT_MIN_WINDOW 8
#define PMD_SHIFT_MAX_DIM 16384
#define PMD_SHIFT_BORDER_NEAREST 0
#define PMD_SHIFT_BORDER_CONSTANT 1
size_t pmd_shift_correlate_workspace_bytes(int n, int d1, int d2, int my, int mx);
int pmd_shift_correlate(pmd_ctx* ctx, const void* X, int elem, long frame_stride, long row_stride, int y0, int x0, int n,
                        int d1, int d2, int my, int mx, const float* tp, float* surf, void* ws, size_t ws_bytes);
int pmd_shift_peak(pmd_ctx* ctx, const float* surf, int n, int my, int mx, int* arg, float* peak, float* neigh);
int pmd_shift_apply(pmd_ctx* ctx, const void* X, int elem, long frame_stride, long row_stride, int n, int d1, int d2,
                    const int* ishift, const float* wts, int border, float fill, void* out, int out_elem,
                    long out_frame_stride, long out_row_stride);

/* Separable spatial filtering of frames (localmd_amd/spatial.py, csrc/spatial.hip): the high-pass that one-photon movies
 * need before template matching, and the band-passed movie their correlation images start from.  X holds n frames of
 * d1 x d2 with the element types and strides of pmd_shift_apply; out likewise.  wy_host holds 2 ry + 1 floats, wx_host
 * 2 rx + 1; both are HOST arrays, read when the call is made and handed to the kernel by value, so there is no device
 * table, no workspace and no synchronisation.  0 <= ry <= min(PMD_FILTER_MAX_RADIUS, d1), rx the same against d2.
 *   a(y, x) = float(f[refl(y)][refl(x)]), refl(i) = -1 - i below 0 and 2 d - 1 - i from d on (SciPy's mode="reflect";
 *     one reflection suffices because r <= d).
 *   Row pass, per source row: h[y][x] is the chain acc = fl(wx[0] a_0), acc = fl(acc + fl(wx[j] a_j)) over ascending j
 *     with a_j = a(y, x + j - rx); s[y][x] is the chain of fp32 adds of the same a_j, ascending.
 *   Column pass: G is the same kind of chain with wy over h[refl(y + i - ry)][x], S the add chain over s.
 *   out = quant(fl(fl(fl(centre a(y, x)) + G) - fl(box S))); the centre term is left out when centre == 0, the box term
 *     and all of s / S when box == 0.  No contraction anywhere; quant is that of pmd_shift_apply (16-bit outputs round
 *     half to even, saturate, NaN -> 0).
 * The bits of an output pixel depend on the frame, the weights and the geometry only: not on n, the strides, the
 * alignment of X / out, the input element type beyond its values, or the tile the pixel falls in.
 * Errors (PMD_ERR_ARG, nothing is launched): n < 0, sides outside 1 .. PMD_SHIFT_MAX_DIM, a radius out of range, an
 * unknown elem / out_elem, a stride shorter than a row or a frame, a NULL pointer, X and out overlapping.  n == 0
 * launches nothing and returns PMD_OK.  The call only enqueues, on the context's stream. */
#define PMD_FILTER_MAX_RADIUS 32
int pmd_spatial_filter(pmd_ctx* ctx, const void* X, int elem, long frame_stride, long row_stride, int n, int d1, int d2,
                       int ry, int rx, const float* wy_host, const float* wx_host, float centre, float box, void* out,
                       int out_elem, long out_frame_stride, long out_row_stride);

/* Piecewise-rigid motion correction (localmd_amd/piecewise.py, csrc/piecewise.hip): patch surfaces around every frame's
 * rigid peak, and the warp by the smooth field the patch shifts span.  max_shift = (my, mx) as above; max_deviation =
 * (ey, ex), each in 1 .. PMD_PATCH_MAX_DEV.  oy = my + ey, ox = mx + ex.
 *
 * Patch area: rows [oy, d1 - oy) x columns [ox, d2 - ox) of the template, Hh x Ww pixels, so that every term of every
 *   patch surface lies inside the frame and every entry sums the same number of terms.
 * Patches: ph x pw pixels, 8 <= ph <= Hh, 8 <= pw <= Ww, at strides 1 <= sy <= ph, 1 <= sx <= pw (no gaps).  Row starts
 *   a_i = min(i sy, Hh - ph) for i < gy = 1 + ceil((Hh - ph) / sy), columns the same; P = gy gx <= PMD_PATCH_MAX.
 *   t'_p is the fp32 template on patch p minus that patch's own mean (float64 on the host, rounded once), packed
 *   (P, ph, pw), p = i gx + j.
 * Patch surfaces: with (cy_k, cx_k) = centre[2 k], centre[2 k + 1] the integer rigid peak of frame k, for 0 <= v <= 2 ey,
 *   0 <= u <= 2 ex
 *     C_{k,p}[v][u] = sum_{i < ph, j < pw} t'_p[i][j] f_k[oy + a_p + i + cy_k + v - ey][ox + b_p + j + cx_k + u - ex],
 *   the un-normalised zero-mean correlation of the patch searched around the frame's own rigid peak.  surf receives
 *   n P (2 ey + 1)(2 ex + 1) floats, frame-major, then patch, then row-major (v, u).  Element types as for
 *   pmd_shift_correlate, widened in registers.  Summation order: a patch is cut into tiles of 32 rows x 64 columns;
 *   inside a tile the rows fall into K = min(32, 256 / (2 ey + 1)) residue classes (row i belongs to class i mod K); an
 *   accumulator is one fmaf chain over the rows of its class ascending, then the columns ascending; the K classes are
 *   added in ascending order, then the tiles in ascending (row-major) order.  No atomics: the bits of a (frame, patch)
 *   surface depend on that frame, t'_p, the centre and the geometry only, not on n, the launch group or the other
 *   patches.  A centre with |cy| > my or |cx| > mx is clamped in the kernel.  ystart (gy ints), xstart (gx ints) and
 *   centre are device tables, so the host cannot see them without synchronising: a start outside 0 .. Hh - ph
 *   (0 .. Ww - pw) is clamped in the kernel as well, it is not an error; no table can cause a read outside the frame.
 *   ws holds the tile partials of a launch group (4 P tiles (2 ey + 1)(2 ex + 1) bytes per frame); the workspace
 *   function sizes it for min(n, 64 MB worth of) frames and any size of at least one frame's partials is taken.
 *   Errors: n < 0, my or mx outside 1 .. PMD_SHIFT_MAX, ey or ex outside 1 .. PMD_PATCH_MAX_DEV, d1 or d2 above
 *   PMD_SHIFT_MAX_DIM, ph or pw below 8 or above the patch area, gy or gx < 1 or gy gx > PMD_PATCH_MAX, an unknown elem,
 *   row_stride < d2, frame_stride < (d1 - 1) row_stride + d2, a NULL X / ystart / xstart / centre / tp / surf
 *   (PMD_ERR_ARG); ws NULL or too small (PMD_ERR_WORKSPACE).
 * Patch peaks: pmd_shift_peak on the n P surfaces with (my, mx) = (ey, ex).  The patch shift is (cy_k + dy_p, cx_k + dx_p)
 *   plus the parabola's offset (host, float64); a patch whose surface has no finite entry, or whose t'_p is all zero,
 *   takes the frame's rigid shift.
 * Field: patch centres yc_i = oy + a_i + (ph - 1) / 2.  Per row y the host gives row_idx[y] = i0 in 0 .. max(gy - 2, 0)
 *   and row_w[y] = ay = clip((y - yc_i0) / (yc_{i0 + 1} - yc_i0), 0, 1) (float64, rounded once; 0 when gy = 1): the field
 *   is constant beyond the outermost centres.  Columns the same.  grid holds per frame the (gy, gx, 2) patch shifts
 *   (dy, dx) in fp32.  The shift of a pixel, per component, every operation rounded on its own:
 *     top = fl(g00 + fl(ax fl(g01 - g00))), bot the same on grid row i0 + 1, s = fl(top + fl(ay fl(bot - top))),
 *   so a grid whose entries are all equal gives exactly that value.  Table indices are clamped to 0 .. g - 2 in the
 *   kernel (and the second index to g - 1).
 * Warp: Y = fl(float(y) + s_y) clamped to [-1, d1], a NaN acting as -1; iy = floor(Y), fy = Y - iy (exact); columns the
 *   same; w00 = fl(fl(1 - fy) fl(1 - fx)), w01 = fl(fl(1 - fy) fx), w10 = fl(fy fl(1 - fx)), w11 = fl(fy fx);
 *   out[y][x] = quant(fl(fl(fl(w00 a) + fl(w01 b)) + fl(fl(w10 c) + fl(w11 d)))) with the samples a, b, c, d at
 *   (iy, ix), (iy, ix + 1), (iy + 1, ix), (iy + 1, ix + 1), their border handling and quant those of pmd_shift_apply; no
 *   contraction, no copy path.  On a frame of finite pixels (none of them -0.0) a grid whose entries are all the same
 *   integer pair gives the bits of pmd_shift_apply for that shift.  Errors: n < 0, sides outside 1 .. PMD_SHIFT_MAX_DIM,
 *   gy or gx outside 1 .. PMD_WARP_MAX_GRID, unknown elem / out_elem / border, a stride shorter than a row or a frame, a
 *   NULL pointer, X and out overlapping (PMD_ERR_ARG).
 * Neither synchronises or allocates; n == 0 launches nothing and returns PMD_OK. */
#define PMD_PATCH_MAX_DEV 7
#define PMD_PATCH_MAX 4096
#define PMD_WARP_MAX_GRID 64
size_t pmd_patch_correlate_workspace_bytes(int n, int d1, int d2, int my, int mx, int ey, int ex, int ph, int pw, int gy,
                                           int gx);
int pmd_patch_correlate(pmd_ctx* ctx, const void* X, int elem, long frame_stride, long row_stride, int n, int d1, int d2,
                        int my, int mx, int ey, int ex, int ph, int pw, int gy, int gx, const int* ystart,
                        const int* xstart, const int* centre, const float* tp, float* surf, void* ws, size_t ws_bytes);
int pmd_warp_apply(pmd_ctx* ctx, const void* X, int elem, long frame_stride, long row_stride, int n, int d1, int d2,
                   const float* grid, int gy, int gx, const int* row_idx, const float* row_w, const int* col_idx,
                   const float* col_w, int border, float fill, void* out, int out_elem, long out_frame_stride,
                   long out_row_stride);

/* A2: background basis = rank-K rSVD of the standardised sample (pmd_loader.py:46-68, :300-314).
 * xs: pixel-major sample with round_up(D,1024) rows allocated (rows >= D zero). basis_out[c][k]. */
size_t pmd_background_rsvd_workspace_bytes(long D, int n, int K);
int pmd_background_rsvd(pmd_ctx* ctx, const float* xs, long D, int n, long ld, int K, uint64_t seed, float* basis_out,
                        void* ws, size_t ws_bytes);

/* A5: temporal projection B^T X (pmd_loader.py:386) and X - B (B^T X) (:387). */
size_t pmd_bg_project_workspace_bytes(long D, int T);
int pmd_bg_project(pmd_ctx* ctx, const float* xs, long D, int T, long ld, const float* basis, int K, float* pj_out,
                   long ldp, void* ws, size_t ws_bytes);
/* pmd_bg_filter: xf_out == xs (in place) is allowed - the pass is element-wise per (pixel, frame). */
int pmd_bg_filter(pmd_ctx* ctx, const float* xs, float* xf_out, long D, int nf, long ld, const float* basis, int K,
                  const float* pj, long ldp);
/* pixel_weighting (decomposition.py:717-718) */
int pmd_scale_rows(pmd_ctx* ctx, float* x, long D, int nf, long ld, const float* w);

/* A4: threshold simulation (decomposition.py:76-131, :147-181).  stats_out[iter][0..1] =
 * (spatial, temporal) roughness of the rank-1 rSVD of an N(0,1) tile; the percentile is host work. */
size_t pmd_threshold_sim_workspace_bytes(int b1, int b2, int t, int iters);
int pmd_threshold_sim(pmd_ctx* ctx, int b1, int b2, int t, int iters, uint64_t seed, float* stats_out, void* ws,
                      size_t ws_bytes);

/* A6-A12: per-tile decomposition, one window (decomposition.py:235-330 single_block_md,
 * evaluation.py:84-222, decomposition.py:501-523).  Omega of tile b is logical array
 * (PMD_STREAM_TILE_OMEGA = 4, omega_index0 + b*omega_index_step).
 * pool_q[P][pool_max]: local pixels of pooling window p (-1 pads); pool_idx[q]: window of pixel q;
 * pool_w[q] = 1/|window|.  n_rows = pixel rows of xf.  Outputs, with rp = pmd_tile_rpad(r): Ut_out[n][rp][dpad],
 * V_out[n][rp][ldv] (= sigma*V rows), stats_out[n][rp][2], good_out/keep_out[n][rp], ranks_out[n], lam_out[n][rp]
 * (sigma^2, may be NULL).  min(r, t_crop / a, P) components exist; the rows from there on are written as zeros in every
 * output (frames < t_crop of V_out).  r is unbounded as in the reference (decomposition.py:643-665); r + 10 > 64 runs the
 * generic-width kernels of wide.hip. */
size_t pmd_tiles_workspace_bytes(int n_tiles, int b1, int b2, int P, int r, int a, int t_crop, long ldv, long n_rows);
int pmd_tiles_decompose(pmd_ctx* ctx, const float* xf, long ldx, long n_rows, int t_crop, const int* tile_pix, int n_tiles, int b1,
                        int b2, const int* pool_q, int pool_max, int P, const int* pool_idx, const float* pool_w, int r,
                        int a, float thr_s, float thr_t, int max_fail, uint64_t seed, uint32_t omega_index0,
                        uint32_t omega_index_step, float* Ut_out, float* V_out, long ldv, float* stats_out,
                        int* good_out, int* keep_out, int* ranks_out, double* lam_out, void* ws, size_t ws_bytes);
/* The same pipeline in three resumable parts, for the reference's denoiser hooks (arbitrary callables inside
 * single_block_md).  stages is a mask: bit 0 = up to V_ds = U_ds^T X_ds (decomposition.py:279-298); the
 * temporal_denoiser (:300) then acts on V_ds[n][rp][ldv] (rows < r, t_crop frames) at byte offset *vds_offset of
 * the workspace; bit 1 = basis of its row space and S = X V_b^T (:301-306); the spatial_denoiser (:310) acts on
 * S[n][rp][dpad] (row c = component c, tile pixel il + b1*jl) at *s_offset; bit 2 = the rest (:315-328 and the
 * keep/discard scan).  The workspace must be left untouched between the calls except for the hook arrays. */
int pmd_tiles_decompose_staged(pmd_ctx* ctx, const float* xf, long ldx, long n_rows, int t_crop, const int* tile_pix, int n_tiles,
                               int b1, int b2, const int* pool_q, int pool_max, int P, const int* pool_idx,
                               const float* pool_w, int r, int a, float thr_s, float thr_t, int max_fail, uint64_t seed,
                               uint32_t omega_index0, uint32_t omega_index_step, float* Ut_out, float* V_out, long ldv,
                               float* stats_out, int* good_out, int* keep_out, int* ranks_out, double* lam_out, void* ws,
                               size_t ws_bytes, int stages);
int pmd_tiles_hook_offsets(int n_tiles, int b1, int b2, int P, int r, int a, int t_crop, long ldv, long n_rows,
                           size_t* vds_offset, size_t* s_offset);

/* A9: one further temporal window (decomposition.py:333-387 single_residual_block_md, :489-515): xw = the
 * window's frames (pixel-major, L frames); Ucur[n][rp][dpad] (rp = pmd_tile_rpad(r)) holds counts[tile] components (other rows zero)
 * and receives the kept components of the residual fit; counts is updated.  pmd_tiles_truncate clears the
 * rows >= counts[tile] of a basis array (after the first window). */
size_t pmd_tiles_residual_workspace_bytes(int n_tiles, int b1, int b2, int r, int a, int L, long n_rows);
int pmd_tiles_residual(pmd_ctx* ctx, const float* xw, long ldx, long n_rows, int L, const int* tile_pix, int n_tiles,
                       int b1, int b2, int r, int a, float thr_s, float thr_t, int max_fail, uint64_t seed,
                       uint32_t omega_index0, uint32_t omega_index_step, float* Ucur, int* counts, float* stats_out,
                       int* good_out, int* keep_out, void* ws, size_t ws_bytes);
int pmd_tiles_truncate(pmd_ctx* ctx, float* U, int dpad, const int* counts, int n_tiles, int rpad);

/* A13: weight and normalise tile bases: Uw = Ut * w[q] / cumw[pix]  (decomposition.py:812-853; csrc/gram.hip). */
int pmd_weight_tiles(pmd_ctx* ctx, const float* Ut, int dpad, const int* tile_pix, int d, const float* w,
                     const float* cumw, const int* ranks, float* Uw_out, int n_tiles);

/* A12/A16: Out[tile] = A[tile] X[tile pixels]  (get_temporal_projector decomposition.py:390-407;
 * the sparse product of pmd_loader.py:411).  A[tile][64][dpad]; Out[tile][64][ldo]. */
int pmd_tiles_project(pmd_ctx* ctx, const float* x, long ldx, int T, const int* tile_pix, int n_tiles, int d,
                      const float* A, int dpad, float* Out, long ldo, int slices);
/* The same when rows >= ranks[tile] of A are zero (the weighted, rank-masked bases of the movie projection): a tile that kept
 * <= 32 components runs half the MFMA work, and rows >= 32 of its Out block are then NOT written (pmd_compact_rows reads
 * rows < rank only). */
int pmd_tiles_project_ranked(pmd_ctx* ctx, const float* x, long ldx, int T, const int* tile_pix, int n_tiles, int d,
                             const float* A, int dpad, float* Out, long ldo, int slices, const int* ranks);
/* Z[col_off[tile] + c][t] = Out[tile][c][t], c < ranks[tile] */
int pmd_compact_rows(pmd_ctx* ctx, const float* Out, long ldo, const int* col_off, const int* ranks, int T, float* Z,
                     long ldz, int n_tiles);

/* A15: G = U^T U for the block-sparse U (decomposition.py:974; csrc/gram.hip); pairs[p] = (tile a, tile b, i0, i1,
 * j0, j1) overlap rectangles, origins[tile] = (k, j).  G is (Rt+K) x (Rt+K), row-major, ldg. */
int pmd_gram_u(pmd_ctx* ctx, const float* Uw, int dpad, int b1, int b2, const int* tile_pix, const int* pairs,
               int n_pairs, const int* origins, const int* col_off, const int* ranks, int n_tiles, int Rt,
               const float* basis, long D, int K, float* G, long ldg);
/* RCCL at this boundary, for a caller that is not built on torch.distributed: one communicator per context,
 * collectives enqueued on the context's stream.  pmd_comm_unique_id: 128 bytes from rank 0, to be broadcast out of band
 * (ncclGetUniqueId); pmd_comm_init: ncclCommInitRank on the context's device; the sharded path needs an in-place fp32
 * sum (partial M^T G M / M^T Z / background projections) and an all-gather of equal-sized blocks
 * (per-tile results).  RCCL is resolved with dlopen at the first call: no link-time dependency, and a process that
 * already holds an RCCL (PyTorch's) shares it.  localmd_amd/parallel.py uses torch.distributed (backend "nccl" = RCCL). */
int pmd_comm_unique_id(void* out128);
int pmd_comm_init(pmd_ctx* ctx, const void* unique_id128, int rank, int world);
int pmd_comm_destroy(pmd_ctx* ctx);
int pmd_comm_all_reduce_f32(pmd_ctx* ctx, float* buf, size_t count);
int pmd_comm_all_gather(pmd_ctx* ctx, const void* send, void* recv, size_t bytes_per_rank);
/* Which eigen-directions pmd_orthogonalize / pmd_orthogonalize_factored keep.  rel_cutoff < 0 (default): the
 * reference's rule - jnp.linalg.svd(hermitian=True) returns |lambda| and u = v sign(lambda), so `eig_vals > 0`
 * (decomposition.py:988) keeps every direction whose eigenvalue is not exactly zero, numerically null ones included.
 * rel_cutoff >= 0: keep lambda > rel_cutoff * lambda_max only ("expose a relative cutoff option"). */
int pmd_ctx_set_null_cutoff(pmd_ctx* ctx, float rel_cutoff);
/* A15: P with (U P)^T (U P) = I (decomposition.py:976-999, only_left=True; csrc/global.hip).  M = right matrix
 * (R x m, NULL = identity, then m = R).  G is overwritten.  *rprime_host = columns kept. */
size_t pmd_orthogonalize_workspace_bytes(int R, int m, int has_m);
int pmd_orthogonalize(pmd_ctx* ctx, float* G, int R, const float* M, int m, long ldm, float* P_out, long ldp,
                      int* rprime_host, void* ws, size_t ws_bytes);
/* A17: projected_svd (decomposition.py:1013-1137).  V: n1 x n2.  nk = min(n1, n2). */
size_t pmd_projected_svd_workspace_bytes(int rows_p, int n1, int n2);
int pmd_projected_svd(pmd_ctx* ctx, const float* P, int rows_p, long ldp, const float* V, int n1, int n2, long ldv,
                      float* R_out, long ldr, float* s_out, float* Vt_out, long ldvt, void* ws, size_t ws_bytes);
/* Block-sparse form of the same Gram matrix, used when R > frames (right_mat = v, decomposition.py:976-981; csrc/gram.hip,
 * the same tile-pair and tile x background sums as pmd_gram_u, stored as blocks):
 * Gblk[pair][64][64], Gbg[kb][tile][64][64] (tile x block kb of 64 background columns; ceil(K / 64) blocks), Gstrip[K][ldgs]
 * (background rows of G).
 * pmd_gram_apply: GM = G M without densifying G.  nbr_ptr[n_tiles+1], nbr[e] = (first M row of the
 * block, rows in it, block index, flags: bit0 transposed, bit1 background block). */
int pmd_gram_blocks(pmd_ctx* ctx, const float* Uw, int dpad, int b1, int b2, const int* tile_pix, const int* pairs,
                    int n_pairs, const int* origins, const int* col_off, const int* ranks, int n_tiles, int Rt,
                    const float* basis, long D, int K, float* Gblk, float* Gbg, float* Gstrip, long ldgs);
int pmd_gram_apply(pmd_ctx* ctx, const float* Gblk, const float* Gbg, const float* Gstrip, long ldgs, const int* nbr_ptr,
                   const int* nbr, const int* col_off, const int* ranks, int n_tiles, int Rt, int K, int max_rank,
                   const float* M, long ldm, int ncols, float* GM, long ldgm);
/* A15/A16/A17 with P = M E^T kept factored (R > frames): Et rows = eigenvectors of M^T G M / sqrt(lambda)
 * (|lambda| descending; which directions are kept: pmd_ctx_set_null_cutoff); then V = Et (M^T Z), its SVD, and
 * R_out = M (Et^T W). */
size_t pmd_orthogonalize_factored_workspace_bytes(int m);
int pmd_orthogonalize_factored(pmd_ctx* ctx, const float* M, int Rc, int m, long ldm, const float* GM, long ldgm,
                               float* Et_out, long lde, int* rprime_host, void* ws, size_t ws_bytes);
/* Cholesky variant of the same step (csrc/chol.hip): Et = U_c^{-T} with M^T G M = U_c^T U_c.  P = M Et^T differs from the
 * eigenvector form by an orthogonal factor that the projected SVD absorbs, so R, s, Vt are unchanged.
 * *ok_host = 0 if the matrix is not numerically positive definite (use pmd_orthogonalize_factored then). */
int pmd_orthogonalize_chol(pmd_ctx* ctx, const float* M, int Rc, int m, long ldm, const float* GM, long ldgm,
                           float* Et_out, long lde, int* ok_host, void* ws, size_t ws_bytes);
size_t pmd_orthogonalize_chol_workspace_bytes(int Rc, int m);
/* The frames x frames part of pmd_projected_svd_factored split by frame columns (multi-GPU: every rank owns T / N columns of
 * W1 = M^T Z; decomposition.py:1089-1099 is the reference step).  pmd_psvd_vp_gram: Vp (rp x nc) = Et (rp x m) W1[:, c0:c0+nc)
 * (W1 points at the first owned column, leading dimension ldw; et_lower: Et is lower triangular) and C = Vp Vp^T (rp x rp,
 * ldc >= round_up(rp, 4), row-major upper triangle) - the caller sums C over the ranks (all-reduce).  pmd_psvd_finish:
 * eigendecomposition of the summed C (every rank the same), s_out (rp), W_out (rp x rp), Vt_out (rp x nc) = this rank's columns
 * of W^T Vp / s.  One rank with nc = T reproduces pmd_projected_svd_factored. */
int pmd_psvd_vp_gram(pmd_ctx* ctx, const float* Et, int rp, int m, long lde, const float* W1, int nc, long ldw, int et_lower, float* Vp,
                     long ldv, float* C, long ldc);
size_t pmd_psvd_finish_workspace_bytes(int rp);
int pmd_psvd_finish(pmd_ctx* ctx, float* C, long ldc, int rp, const float* Vp, int nc, long ldv, float* W_out, long ldw, float* s_out,
                    float* Vt_out, long ldvt, void* ws, size_t ws_bytes);
size_t pmd_projected_svd_factored_workspace_bytes(int Rc, int m, int rp, int T);
int pmd_projected_svd_factored(pmd_ctx* ctx, const float* M, int Rc, int m, long ldm, const float* Et, int rp, long lde,
                               const float* Z, int T, long ldz, float* R_out, long ldr, float* s_out, float* Vt_out,
                               long ldvt, float* Vp_out, long ldvp, float* X1_out, const float* W1_in, int et_lower,
                               void* ws, size_t ws_bytes);
/* (X1_out: optional m x rp, ld rp, receives Et^T W.  With R_out == NULL the last product R = M X1 is left to the
 * caller, who can then form R in row blocks with pmd_gemm and overlap their download with the next block.
 * W1_in: optional m x T, ld T: M^T Z formed by the caller, e.g. the all-reduced sum of per-rank row-range partials.
 * et_lower != 0: Et is square lower triangular (pmd_orthogonalize_chol / pmd_chol_inverse), strmm replaces two GEMMs.) */
/* The two halves of pmd_orthogonalize_chol (csrc/chol.hip), for callers that shard the rows of M over ranks: the partial
 * C = M[rows]^T GM[rows] (row-major lower block triangle; all-reduce it), then C -> Et in place. */
size_t pmd_gram_mtgm_workspace_bytes(int rows, int m);
/* leading dimension of the transposed copy M^T (m x rows) that pmd_gram_mtgm leaves at the start of its workspace (a multiple
 * of 64 floats; the host driver reuses the copy for the M^T Z product) */
long pmd_gram_mtgm_ld(int rows);
int pmd_gram_mtgm(pmd_ctx* ctx, const float* M, int rows, int m, long ldm, const float* GM, long ldgm, float* C, long ldc,
                  void* ws, size_t ws_bytes);
size_t pmd_chol_inverse_workspace_bytes(int m);
/* abs_last_pivot != 0: the caller has rotated a known null direction of C into the last row / column; a negative last
 * pivot is then replaced by its absolute value instead of failing - the Cholesky-route form of the reference keeping
 * numerically null directions through |lambda| (svd(hermitian=True) at decomposition.py:984, `eig_vals > 0` at :988). */
int pmd_chol_inverse(pmd_ctx* ctx, float* C, int m, long ldc, int abs_last_pivot, int* ok_host, void* ws, size_t ws_bytes);
/* dst (cols x rows, ld_dst) = src (rows x cols, ld_src)^T, row-major */
int pmd_transpose(pmd_ctx* ctx, const float* src, long ld_src, int rows, int cols, float* dst, long ld_dst);
/* A13/A14: CSR arrays of the sparse spatial matrix built on the device (decomposition.py:812-853, :929-930; csrc/gram.hip);
 * cover1[d1][4] / cover2[d2][4]: indices of the tile-row / tile-column origins covering each FOV row / column. */
int pmd_csr_count(pmd_ctx* ctx, int d1, int d2, int order_f, const int* cover1, const int* cover2, int n2,
                  const int* ranks, int K, long* row_nnz);
int pmd_csr_fill(pmd_ctx* ctx, int d1, int d2, int order_f, int b1, const int* cover1, const int* cover2,
                 const int* orig1, const int* orig2, int n2, const int* ranks, const int* col_off, const float* Ut,
                 int dpad, const float* w, const double* inv_cumw, const float* basis, int K, int Rt, const long* indptr,
                 double* data, int* indices, int* zero_count, int rpad);   /* rpad: component rows of Ut (pmd_tile_rpad) */
/* row-major C = alpha op(A) op(B) + beta C (the jnp.matmul calls of decomposition.py:873, :982, :993,
 * :1006; pmd_loader.py:412) */
int pmd_gemm(pmd_ctx* ctx, int transA, int transB, int m, int n, int k, float alpha, const float* A, long lda,
             const float* B, long ldb, float beta, float* C, long ldc);
/* 1 when pmd_gemm runs a product of this size as three fp16-piece products on the fp16 matrix cores (csrc/gemm_f16x2.hip:
 * fp32 operands and result, error below the sgemm path's; PMD_GEMM_SPLIT=0 switches it off).  Those products accumulate
 * into C, so C should then live in HBM (a host-mapped C takes the sgemm path). */
int pmd_gemm_split_active(pmd_ctx* ctx, int m, int n, int k);
/* Frees the library-owned device scratch of the large products (fp16 pieces, split-K partial sums) when it is larger than
 * keep_bytes; it is re-created on demand.  The host driver calls it at the end of every decomposition. */
int pmd_scratch_trim(pmd_ctx* ctx, size_t keep_bytes);

/* A18: expansion back into pixels (pmdarray.py:132-171, PMDArray.__getitem__: spatial.dot(temporal), times the
 * noise image, plus the mean image, frames first).  pmd_csr_rows_spmm: out[p][f] = sum over the nonzeros i of CSR
 * row rows[p] (rows == NULL: row p) of data[i] * B[indices[i]][f], f < ncols; B is the dense (R diag(s)) Vt[:, frames]
 * or R diag(s).  pmd_transpose_affine: dst[c][r] = src[r][c] * scale[r] + shift[r] (scale / shift may be NULL). */
int pmd_csr_rows_spmm(pmd_ctx* ctx, const int64_t* indptr, const int* indices, const float* data, const int* rows, long n_sel,
                      const float* B, long ldb, int ncols, float* out, long ldo);
/* SURVEY 8(f)4 - the local correlation images of /root/reference/localmd/diagnostic_plots.py (their O(D) Python loops of
 * jitted per-pair calls, :131-156, :195-221, :247-268, :293-302) from first and second moments of the pixel traces.
 * Movies are frames first (T, d1, d2) float32 on the device; ref[D] = one frame of the movie (the traces are shifted by it,
 * covariances do not change).  pmd_neighbour_moments: moments[10][D] (+)= {sum x, sum x^2, sum x_p x_q for the 8 neighbours
 * q in row-major (di, dj) order} of x = A - B (B may be NULL); call it once per resident chunk of frames with accumulate = 1
 * after the first.  pmd_neighbour_image: kind 0 = Pearson correlation (make_correlation_image), kind 1 = cov(ddof 1) of the
 * numerator movie over sqrt(var var) (ddof 0) of the normalising movie `den` = its moments[0..1] (make_pmd_correlation_image,
 * make_residual_correlation_image); mode 0 = max over the existing neighbours starting from 0, mode 1 = their mean.
 * pmd_lag_moments / pmd_lag_image: make_autocorrelation_image; moments[5][D] (+)= sums over the pairs (t, t - lag), t in
 * [lag, T) of the resident frames (a chunk therefore starts `lag` frames before its first new frame); n = T_total - lag. */
size_t pmd_diag_workspace_bytes(long T, long D);
int pmd_neighbour_moments(pmd_ctx* ctx, const float* A, const float* B, const float* ref, long T, int d1, int d2, int accumulate,
                          double* moments, void* ws, size_t ws_bytes);
int pmd_lag_moments(pmd_ctx* ctx, const float* A, const float* ref, long T, long D, int lag, int accumulate, double* moments,
                    void* ws, size_t ws_bytes);
int pmd_neighbour_image(pmd_ctx* ctx, const double* num, const double* den, long T, int d1, int d2, int kind, int mode, double* out);
int pmd_lag_image(pmd_ctx* ctx, const double* moments, long D, long n, double* out);
/* One-pass fit diagnostics (localmd_amd.diagnostic_images.make_pmd_diagnostic_images): the moments behind all four
 * images of diagnostic_plots.py and the residual statistics from one read of the movie.  Per call, frames [c0, c0 + n)
 * of a frames-first batch Y (element type elem, row 0 = frame ybase <= c0; converted to fp32) and of W (n x D fp32,
 * row 0 = frame c0), the reconstruction std * (U R diag(s) Vt) without the mean; mean[D] = the decomposition's mean
 * image.  With the residual r = (y - mean) - w: moments[35][D] += {neighbour moments of y (10), of w (10), of r (10),
 * in the layout of pmd_neighbour_moments; lag moments of y (5) in the layout of pmd_lag_moments}, frame_ss[c0 + f] =
 * sum over the pixels of r^2 (frame_ss has T entries).  Traces are shifted by their values in frame 0: ref[3][D] is
 * written by the call with c0 = 0, which must come first.  c0 is a multiple of 512 and the calls come in frame order,
 * so the fp64 sums are bitwise independent of the batching.  A lag pair whose earlier frame is before ybase reads it
 * from ring (lag x D, element type elem, slot = frame mod lag), which the caller fills from the earlier batches.
 * Finish with pmd_neighbour_image (kind 0 on moments, kind 1 on moments + 10 D / + 20 D with den = moments) and
 * pmd_lag_image(moments + 30 D, n = T - lag).  No synchronisation, no allocation. */
size_t pmd_diag_fused_workspace_bytes(int n, long D);
int pmd_diag_fused_accumulate(pmd_ctx* ctx, const void* Y, int elem, long ybase, const float* W, const void* ring, int lag,
                              long c0, int n, long T, int d1, int d2, const float* mean, float* ref, double* moments,
                              double* frame_ss, void* ws, size_t ws_bytes);
int pmd_transpose_affine(pmd_ctx* ctx, const float* src, long lds_, long rows, int cols, const float* scale,
                         const float* shift, float* dst, long ldd);

/* ---- kernel-level entry points (used by the parity tests; same kernels as above) ---------- */
/* The four contractions of csrc/tile_gemm.hip.  Every per-tile [comp][x] array has 64 rows, all of which exist.  Pixel q of
 * a tile is row pix[tile * pix_stride + q] of X (entries q >= d of a pix row are never looked at), or row
 * tile * row0_stride + q when pix is NULL.  X and every per-tile array are 16-byte aligned with leading dimensions and tile
 * strides that are multiples of 4 floats, unless a paragraph says otherwise.  tests/test_gpu_tile_contractions.py pins what
 * follows.
 *
 * tile_atx:  Out[tile][c][t] = sum_{q < d} A[tile][c][q] X[pixel q][t],  c < 64, t < T.
 *   A[tile][64][a_ld], a_ld >= pmd_tile_dpad(d), columns [d, pmd_tile_dpad(d)) ZERO (they meet pixel rows that are not the
 *   tile's); a_tile_stride 0 shares one A between the tiles.
 *   X is read in whole chunks of 32 frames: frames [0, round_up(T, 32)) of every pixel row are read (ldx at least that).  What
 *   they hold from T on need not be zero, it only reaches the output columns of the same index.  For 256 < d <= 400 and
 *   ldx >= 32 (ceil(T / 32) + 2) - pmd_time_ld(T) is - the LDS-DMA kernel runs and also fetches, and drops, up to two chunks
 *   behind the last one; with a shorter ldx, or PMD_ATX_DMA=0, the register-staged kernel of the same shape runs.
 *   Out[tile][64][ldo], ldo >= round_up(T, 32): all 64 rows, columns [0, round_up(T, 32)) are written, those from T on with
 *   whatever the padding of X gives.  For d <= 1024 no other column is touched.  For d > 1024 the slices of 1024 pixels add
 *   up by atomicAdd: the whole 64 x ldo block of every tile is cleared first, so columns from round_up(T, 32) on end as
 *   zeros (no driver keeps anything there), and the rounding order, hence the last bit, may differ from run to run.
 *   slices: the chunks are dealt to at most this many workgroups per tile. */
int pmdk_tile_atx(pmd_ctx* ctx, const float* X, long ldx, const int* pix, int pix_stride, long row0_stride, int d,
                  const float* A, long a_tile_stride, int a_ld, float* Out, long out_tile_stride, long ldo, int n_tiles,
                  int T, int slices);
/* the same with the number of rows of A that carry data (rows >= `rows` are zero): <= 16 rows on tiles of 801 to 1024
 * pixels run a specialised kernel that leaves rows >= 16 of Out unwritten; any other hint changes nothing */
int pmdk_tile_atx_rows(pmd_ctx* ctx, const float* X, long ldx, const int* pix, int pix_stride, long row0_stride, int d,
                       const float* A, long a_tile_stride, int a_ld, float* Out, long out_tile_stride, long ldo, int n_tiles,
                       int T, int slices, int rows);
/* tile_xbt:  sum_slice S[tile][slice][c][q] = sum_{t < T} B[tile][c][t] X[pixel q][t],  c < 64, q < d.
 *   B[tile][64][ldb] (b_tile_stride 0: shared).  Both operands are read in whole groups of 16 frames and nothing is masked
 *   along time: frames [0, round_up(T, 16)) of the d pixel rows and of all 64 rows of B are read, nothing behind them.  In
 *   frames [T, round_up(T, 16)) X must be ZERO - the drivers clear every movie copy behind its last fitted frame - and B must
 *   be finite; B need not be zero there (a trace array keeps there whatever tile_atx left).
 *   S[tile][slices][64][s_ld], s_ld >= 16 ceil(d / 16): the frame groups are dealt to at most `slices` slices and the caller
 *   sums all the slices it asked for.  A slice with work gets rows 0..63, columns [0, 16 ceil(d / 16)), zeros in columns
 *   >= d, and keeps the rest of its rows; slices without work (there are fewer frame groups than slices, or their rounded-up
 *   share leaves the last slices none: T = 133 on four slices fills three) are cleared over their whole s_slice_stride.
 *   s_slice_stride 0 is for slices = 1. */
int pmdk_tile_xbt(pmd_ctx* ctx, const float* X, long ldx, const int* pix, int pix_stride, long row0_stride, int d,
                  const float* B, long b_tile_stride, long ldb, float* S, long s_tile_stride, long s_slice_stride,
                  int s_ld, int n_tiles, int T, int slices);
/* tile_gram:  sum_slice G[tile][slice][i][j] = sum_{x < len} In[tile][i][x] In[tile][j][x]  in fp64,  i, j < 64.
 *   In[tile][64][ld], ld >= len: all 64 rows are read, never outside [0, ld) of a row, and positions >= len are masked: they
 *   may hold anything, NaN included.  Any ld, tile_stride and alignment is served (the fp64-MFMA kernel needs ld % 4 == 0,
 *   ld >= 16, tile_stride % 4 == 0 and a 16-byte aligned base; the scalar kernel takes the rest, and everything under
 *   PMD_GRAM_MFMA=0).
 *   G[tile][slices][64][64] doubles: every slice is written in full; slice s covers positions
 *   [s c, (s + 1) c), c = round_up(ceil(len / slices), 32), and is zero when that range is empty.  The sum over the slices
 *   is symmetric to the bit. */
int pmdk_tile_gram(pmd_ctx* ctx, const float* In, long tile_stride, long ld, int len, int n_tiles, int slices,
                   double* G);
/* tile_rowmix:  Out[tile][c][x] = (float) sum_{c' < n_in} N[tile][c'][c] In[tile][c'][x]  (fp64 sum, one rounding),
 *   c < n_out, x < len; rows [n_out, 64) of Out are set to zero up to len; nothing from len on is written.
 *   N[tile][64][64] doubles (n_tile_stride 0: shared): the whole block is read, entries outside n_in x n_out are masked.
 *   In[tile][64][ld_in]: all 64 rows are read, rows >= n_in masked; positions < len, and in the 64-position MFMA kernel
 *   < round_up(len, 4) (it runs only when ld_in holds them), those from len on without effect.  Masked entries may hold
 *   anything, NaN included.  Out == In with equal strides is allowed.  Any ld and alignment is served: without 16-byte
 *   aligned rows, or with len < 4, the 64-position kernel gives way to the 16-position one. */
int pmdk_tile_rowmix(pmd_ctx* ctx, const float* In, long in_tile_stride, long ld_in, const double* N,
                     long n_tile_stride, int n_in, int n_out, float* Out, long out_tile_stride, long ld_out, int len,
                     int n_tiles);
/* The other kernels of the 64-row main path (csrc/small_la.hip and the pooling part of csrc/prep.hip).
 * tests/test_gpu_tile_small_la.py pins the four paragraphs that follow; tests/small_la_ref.py derives their bounds.
 *
 * small_qr:  Qt[tile][c][q] = Q[q][c] of the reduced Householder QR of the P x l matrix Y[q][c] = Yt[tile][c][q],
 *   c < nref = min(P, l), q < P, with LAPACK's conventions (dgeqr2 + dorg2r: beta = -sign(alpha) norm), so that on a matrix
 *   of full rank the columns agree with LAPACK's sign included.  One workgroup per tile.
 *   Read: rows c < l, columns q < P of every Yt tile, nothing else (any y_ld >= P, any y_tile_stride, no alignment).
 *   Written: rows c < nref, columns q < P of every Qt tile.  Rows [nref, 64), columns [P, q_ld) and whatever lies between
 *   the tiles are left alone: a caller that wants zeros there clears the buffer first.
 *   Storage: the matrix is held in LDS with the odd leading dimension ldm = P | 1, in fp64 while
 *   l ldm 8 + 2608 <= 150 KB (l = 60: P <= 313), in fp32 beyond that (every store to it then rounds to fp32; the arithmetic
 *   stays fp64), and l ldm 4 + 2608 <= 160 KB must hold (l = 64: P <= 629).  l > 64 or a matrix that does not fit:
 *   PMD_ERR_UNSUPPORTED, nothing is launched or written, the context stays usable.
 *   Dependence rule: a column of which, after the earlier reflectors, no more than left^2 <= dep_tol |column as loaded|^2
 *   remains (dep_tol 1e-24 in fp64 storage, 1e-12 in fp32 storage), or exactly nothing below its diagonal, gets tau = 0: its
 *   Q column is the unit vector under the earlier reflectors.  Q has nref orthonormal columns whatever the rank, and Y = Q Q^T Y
 *   up to sqrt(dep_tol) of a column's norm.  The rule is relative and every operation is exact under a power-of-two scale:
 *   Y 2^k gives the same bits (short of overflow and underflow). */
int pmdk_small_qr(pmd_ctx* ctx, const float* Yt, long y_tile_stride, int y_ld, int P, int l, float* Qt,
                  long q_tile_stride, int q_ld, int n_tiles);
/* small_eig:  eigendecomposition of M[tile] = 1/2 sum_k (G_k + G_k^T), the leading n x n blocks of the `slices` 64 x 64
 *   blocks of G[tile][slices][64][64] summed in their order and symmetrised; 1 <= n <= 64 (else PMD_ERR_UNSUPPORTED).
 *   Read: the leading n x n block of every slice, nothing outside it (the default kernel; under PMD_SMALL_EIG=rocsolver the
 *   batch goes through pmdk_wide_eig at rp = 64, which reads the same entries).  The block must be FINITE: a NaN or Inf in
 *   it is not detected and the output is then undefined.
 *   Written: all of Nout[tile][64][64] and lam_out[tile][64].  lam_out[c], c < n: the eigenvalues in descending order;
 *   Nout[c'][c]: component c' of the eigenvector of lam_out[c]; exact zeros outside n x n and in lam_out from n on.
 *   mode 0: the orthonormal eigenvectors.
 *   mode 2: the same columns, those with lam_c <= tol lam_0 or lam_c <= 0 zeroed (lam_0 is the largest eigenvalue, signed:
 *           a matrix without a positive eigenvalue gives all zeros; tol = 0 still drops every non-positive direction).
 *   mode 1: the kept columns of mode 2 times 1 / sqrt(lam_c): N^T M N = I on them.
 *   The rule is applied to the eigenvalues as returned, so an eigenvalue that is zero in exact arithmetic and comes out as
 *   +1e-17 lam_0 is kept at tol = 0; callers pass a tol well above the solver's accuracy (1e-12 max|lam| absolute).
 *   Default kernel: one wave per problem, Householder tridiagonalisation (a column with nothing below its subdiagonal
 *   is passed over: diagonal and tridiagonal input), Q formed in place, implicit QL with accumulated rotations.  Kept
 *   columns of mode 2 are those of mode 0 bit for bit, those of mode 1 differ from column / sqrt(lam) by three roundings. */
int pmdk_small_eig(pmd_ctx* ctx, const double* G, int slices, int n, int mode, double tol, double* Nout,
                   double* lam_out, int n_tiles);
/* Cholesky whitening of the 64-row path: G[tile][slices][64][64], Nout[tile][64][64] = inverse of the upper factor of the
 * symmetrised slice sum's leading n x n block; a pivot <= tol * max diagonal gives a zero column; zero outside n x n. */
int pmdk_small_chol(pmd_ctx* ctx, const double* G, int slices, int n, double tol, double* Nout, int n_tiles);
/* generic width (rp a multiple of 64): G[tile][slices][rp][rp] = In In2^T over `slices` position ranges (In2 NULL: In) */
int pmdk_wide_gram(pmd_ctx* ctx, const float* In, long tile_stride, long ld, int len, int n_tiles, int slices, int rp,
                   double* G, const float* In2);
/* workspace of pmdk_wide_eig for n_tiles problems of order n */
size_t pmdk_wide_eig_workspace_bytes(int n, int n_tiles);
/* pmdk_small_eig at any rp: G[tile][slices][rp][rp], Nout[tile][rp][rp], lam_out[tile][rp], order n <= rp (rocSOLVER) */
int pmdk_wide_eig(pmd_ctx* ctx, const double* G, int slices, int rp, int n, int mode, double tol, double* Nout,
                  double* lam_out, int n_tiles, void* ws, size_t ws_bytes);
/* pmdk_tile_rowmix at any rp: N[tile][rp][rp] (n_tile_stride 0: shared); rows [n_out, rp) of Out are zeroed up to len */
int pmdk_wide_rowmix(pmd_ctx* ctx, const float* In, long in_tile_stride, long ld_in, const double* N, long n_tile_stride,
                     int rp, int n_in, int n_out, float* Out, long out_tile_stride, long ld_out, int len, int n_tiles);
/* tile_pool_bin:  xbar[c][cb] = mean_{tau < a} X[c][a cb + tau],  c < n_rows, cb < nbins  (scratch, ld_ab floats a row);
 *   abar[tile][p][cb] = mean over the pixels q of window p of xbar[pix[tile d + q]][cb],  p < P, cb < nbins, where window p
 *   is the entries >= 0 of pool_q[p][0 .. pool_max) (local pixel ids, -1 = padding; every window has at least one pixel).
 *   Read: frames [0, a nbins) of the n_rows rows of X - frames behind them, the remainder of T / a included, are never
 *   read -, all of pix and pool_q.  Written: columns [0, nbins) of rows [0, n_rows) of xbar and of rows [0, P) of every abar
 *   tile (abar[tile] starts at tile * tile_stride, row p at p * ld_ab); columns from nbins on, rows of xbar from n_rows on
 *   and whatever lies between the tiles are left alone.  Any n_rows, n_tiles and nbins (launch chunks of 32768 rows / tiles,
 *   a grid-stride loop over the bins).
 *   Summation order, fp32 throughout: a bin is summed frame by frame from zero and multiplied by the rounded 1 / a; a window
 *   is summed in the order of pool_q from zero and multiplied by the rounded 1 / count.  Hence
 *   |xbar - exact| <= (a + 1) 2^-24 mean|x| and |abar - exact| <= (a + count + 2) 2^-24 (window mean of the bin means of |x|),
 *   and small integers with a and every count a power of two come out exact. */
int pmdk_tile_pool_bin(pmd_ctx* ctx, const float* X, long ldx, long n_rows, const int* pix, int n_tiles, int d,
                       const int* pool_q, int pool_max, int P, int a, int nbins, float* xbar, float* abar, long ld_ab,
                       long tile_stride);
/* roughness:  stats[tile][c][0] = spatial, stats[tile][c][1] = temporal roughness statistic of component c < r
 *   (evaluation.py:84-126): the mean absolute difference of vertical and horizontal neighbours of the b1 x b2 image
 *   Ut[tile][c][i + b1 j] over the mean absolute pixel, and mean_{0 < t < T - 1} |v[t-1] + v[t+1] - 2 v[t]| over mean_t |v[t]|
 *   of the trace v = V[tile][c][.].  An all-zero row gives NaN (0 / 0), as the reference does; T >= 3 and b1 b2 >= 2.
 *   Read: columns [0, b1 b2) of rows c < r of Ut, columns [0, T) of rows c < r of V; nothing behind them, no other row.
 *   Written: stats[tile][c][.] for c < r only, rows [r, 64) are left alone (the keep/discard scan clears them); with
 *   Ut == NULL only the temporal, with V == NULL only the spatial statistic is written.
 *   Summation order, fp32 throughout: spatial - one wave, lane k adds the terms of pixels k, k + 64, .. (ceil(b1 b2 / 64)
 *   terms), six butterfly steps, then sum of the two difference sums, the two divisions by the counts and the quotient;
 *   temporal - 256 threads, thread k adds frames k, k + 256, .., six butterfly steps in each wave, (w0 + w1) + (w2 + w3)
 *   across the waves, the two divisions by T - 2 and T and the quotient.  The second difference is formed as
 *   (v[t-1] + v[t+1]) - 2 v[t]: its rounding error is absolute in |v|, 2^-24 |v[t-1] + v[t+1]|, not relative to the result. */
int pmdk_roughness(pmd_ctx* ctx, const float* Ut, long u_tile_stride, int u_ld, int b1, int b2, const float* V,
                   long v_tile_stride, long v_ld, int T, int r, float* stats, int n_tiles);
int pmdk_syevd(pmd_ctx* ctx, int n, float* A, long lda, float* w, float* work, int* info);
/* Householder tridiagonalisation A = Q T Q^T with LAPACK ssytrd('L') conventions on the column-major view
 * of the buffer (memory row c holds A(r, c), r >= c, at offset r): d[n], e[n-1], tau[n-1], reflectors in A.
 * impl 0 = rocSOLVER, 1 = the library's own kernels (lda % 4 == 0, lda >= round_up(n, 4)). */
int pmdk_sytrd(pmd_ctx* ctx, int n, float* A, long lda, float* d, float* e, float* tau, int impl);
/* stage 1 of the two-stage reduction (sytrd2.hip): dense -> band of half bandwidth 64; reflectors of Q1 below the band
 * (unit entry of reflector c at position c + 64), tau1[n]; *flag_host != 0: a panel was rank deficient, A is handed
 * back as it came */
int pmdk_sy2sb(pmd_ctx* ctx, int n, float* A, long lda, float* tau1, int* flag_host);
/* stages 1 + 2: dense -> band -> tridiagonal (bulge chasing); d[n], e[n - 1] on the device */
int pmdk_sytrd2(pmd_ctx* ctx, int n, float* A, long lda, float* tau1, float* d, float* e, int* flag_host);

#ifdef __cplusplus
}
#endif
#endif
