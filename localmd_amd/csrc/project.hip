// Projection of raw frames onto a stored spatial basis (pmd_loader.py:316-346 v_projection, :393-414
// v_projection_routine):  Z[row][f] = sum_q A_g[row][q] * (Y[f][pix_g[q]] - mean) / std  for every group g of the
// columns of U (localmd_amd/projection.py builds the groups: the tiles of a decomposition, found as runs of consecutive
// columns on a common support of at most P_MAX pixels, and the pixel chunks of the wide background columns).
//
// One workgroup = one group x one block of 64 frames.  The group's pixels are walked in chunks of 64: every chunk is
// standardised while it is staged into LDS (Xs[frame][q], the fp32 expression of standardize_transpose_kernel, so the
// staged values are bitwise the ones of the two-pass route) next to the matching 64 columns of A_g (As[row][q]), and the
// four waves contract the two tiles on v_mfma_f32_16x16x4_f32.  Only the row tiles of 16 that hold rows of the group
// are computed (a group of 21 rows costs two row tiles, not four), and frame tiles beyond n are skipped.
// The sum over the pixels of a group is one k-ordered fp32 fma chain whose order depends only on the group table, and
// the MFMA computes every output column on its own, so Z[:, f] does not depend on n or on the batch frame f arrives in.
// Groups of wide columns write partial sums to the workspace; group_reduce_kernel adds them in chunk order (no atomics).
//
// Grid: workgroup id = g * n_frame_blocks + frame block.  The frame blocks of one group are neighbours in the launch
// order, so A_g (read once per workgroup, up to 64 x 1600 fp32) is served by L2 for all but the first block on each XCD.
#include "pmd_common.h"
#include "../../include/pmd_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int PJ_FB = 64;          // frames per workgroup
constexpr int PJ_KC = 64;          // pixels per LDS chunk
constexpr int PJ_LS = PJ_KC + 4;   // LDS row stride (floats): lane (i = l & 15, k = l >> 4) reads bank 4 i + k, conflict-free
constexpr int PJ_GT = 6;           // int64 entries per group of the table

template <typename E>
__global__ __launch_bounds__(256) void group_project_kernel(const E* __restrict__ Y, int n, long D,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ stdv,
                                                            const long* __restrict__ groups, int n_fb,
                                                            const int* __restrict__ pix, const float* __restrict__ A,
                                                            float* __restrict__ Z, long ldz, float* __restrict__ ws) {
  __shared__ float Xs[PJ_FB][PJ_LS];
  __shared__ float As[PMD_RPAD][PJ_LS];
  const long g = (long)blockIdx.x / n_fb;
  const int f0 = (int)((long)blockIdx.x - g * n_fb) * PJ_FB;
  const long* gt = groups + g * PJ_GT;
  const long pix_off = gt[0], a_off = gt[2], out_row = gt[3];
  const int p = (int)gt[1], r = (int)gt[4], to_ws = (int)gt[5];
  const int rt_n = (r + 15) >> 4;                       // row tiles with data (A_g holds rt_n * 16 rows)
  const int ft_n = min(PJ_FB, n - f0 + 15) >> 4;        // frame tiles with at least one frame < n
  const int p64 = (p + PJ_KC - 1) / PJ_KC * PJ_KC;      // row length of A_g
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int li = lane & 15, lk = lane >> 4;
  const int n_pairs = rt_n * ft_n;                       // (row tile, frame tile) pairs, dealt to the waves round-robin
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int q0 = 0; q0 < p; q0 += PJ_KC) {
    // stage: thread (q = lane, frames w + 4u) -- a wave reads 64 consecutive pixel ids of one frame (runs of b2
    // contiguous pixels).  Loads are unconditional on clamped indices and the value is masked afterwards.
    {
      const int q = q0 + lane;
      const bool qv = q < p;
      const long c = pix[pix_off + (qv ? q : 0)];
      const float mu = mean[c];
      const float sg = stdv[c];
      float y[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int f = min(f0 + w + 4 * u, n - 1);
        y[u] = (float)Y[(long)f * D + c];
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int fl = w + 4 * u;
        Xs[fl][lane] = (qv && f0 + fl < n) ? (y[u] - mu) / sg : 0.f;
      }
      for (int rr = w; rr < rt_n * 16; rr += 4) As[rr][lane] = A[a_off + (long)rr * p64 + q];
    }
    __syncthreads();
    int j = 0;
    for (int pr = w; pr < n_pairs; pr += 4, ++j) {
      const int rt = pr % rt_n, ft = pr / rt_n;
      const float* arow = &As[rt * 16 + li][lk];
      const float* brow = &Xs[ft * 16 + li][lk];
      f32x4 a_acc = acc[0];
      if (j == 1) a_acc = acc[1];
      if (j == 2) a_acc = acc[2];
      if (j == 3) a_acc = acc[3];
#pragma unroll
      for (int s = 0; s < PJ_KC / 4; ++s) a_acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[4 * s], brow[4 * s], a_acc, 0, 0, 0);
      if (j == 0) acc[0] = a_acc;
      if (j == 1) acc[1] = a_acc;
      if (j == 2) acc[2] = a_acc;
      if (j == 3) acc[3] = a_acc;
    }
    __syncthreads();
  }

  // C/D map of 16x16x4: column = lane & 15, rows (lane >> 4) * 4 + v
  float* out = to_ws ? ws : Z;
  const long ld = to_ws ? (long)n : ldz;
  int j = 0;
  for (int pr = w; pr < n_pairs; pr += 4, ++j) {
    const int rt = pr % rt_n, ft = pr / rt_n;
    const int f = f0 + ft * 16 + li;
    f32x4 v = acc[0];
    if (j == 1) v = acc[1];
    if (j == 2) v = acc[2];
    if (j == 3) v = acc[3];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = rt * 16 + lk * 4 + e;
      if (row < r && f < n) out[(out_row + row) * ld + f] = v[e];
    }
  }
}

// Z[z_row][f] = sum_{c < parts} ws[ws_row0 + c * stride][f], c ascending.
__global__ __launch_bounds__(256) void group_reduce_kernel(const long* __restrict__ wide, int n,
                                                           const float* __restrict__ ws, float* __restrict__ Z, long ldz) {
  const long* wt = wide + (long)blockIdx.y * 4;
  const long z_row = wt[0], row0 = wt[1], stride = wt[3];
  const int parts = (int)wt[2];
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n) return;
  float s = 0.f;
  for (int c = 0; c < parts; ++c) s += ws[(row0 + c * stride) * n + f];
  Z[z_row * ldz + f] = s;
}

}  // namespace

extern "C" {

size_t pmd_group_project_workspace_bytes(long n_partial_rows, int n) {
  if (n_partial_rows <= 0 || n <= 0) return 0;
  return (size_t)n_partial_rows * (size_t)n * sizeof(float);
}

int pmd_group_project(pmd_ctx* ctx, const void* Y, int elem, int n, long D, const float* mean, const float* std,
                      int n_groups, const long* groups, const int* pix, const float* A, long n_partial_rows,
                      int n_wide_rows, const long* wide, float* Z, long ldz, void* ws, size_t ws_bytes) {
  CTX_CHECK(ctx);
  const char* what = "pmd_group_project";
  if (n < 0 || D < 1 || n_groups < 0 || n_wide_rows < 0 || n_partial_rows < 0 || ldz < n)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (n >= 0, D >= 1, counts >= 0, ldz >= n)");
  if (pmd_bad_elem(elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown element type");
  if ((n_wide_rows > 0) != (n_partial_rows > 0))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "partial rows and wide rows come together");
  if (n == 0 || n_groups == 0) return PMD_OK;
  if (!Y || !mean || !std || !groups || !pix || !A || !Z || (n_wide_rows > 0 && !wide))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if (ws_bytes < pmd_group_project_workspace_bytes(n_partial_rows, n) || (n_partial_rows > 0 && !ws))
    return pmd_fail(ctx, PMD_ERR_WORKSPACE, what, "workspace too small");
  const long n_fb = ((long)n + PJ_FB - 1) / PJ_FB;   // (in long: n + 63 overflows an int from 2^31 - 64 on)
  if ((long)n_groups * n_fb > 0x7fffffffL) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many groups x frame blocks");
  pmd_prof_scope prof__(ctx, "group_project");
  const dim3 grid((unsigned)((long)n_groups * n_fb));
  float* wsf = (float*)ws;
  pmd_with_elem(elem, [&](auto e) {
    using E = typename decltype(e)::type;
    hipLaunchKernelGGL(group_project_kernel<E>, grid, dim3(256), 0, ctx->stream, (const E*)Y, n, D, mean, std, groups,
                       (int)n_fb, pix, A, Z, ldz, wsf);
  });
  PMD_LAUNCH_CHECK(ctx, "group_project_kernel");
  if (n_wide_rows > 0) {
    for (int r0 = 0; r0 < n_wide_rows; r0 += 65535) {
      const int rn = (n_wide_rows - r0 < 65535) ? n_wide_rows - r0 : 65535;
      hipLaunchKernelGGL(group_reduce_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)rn), dim3(256), 0, ctx->stream,
                         wide + (long)r0 * 4, n, wsf, Z, ldz);
    }
    PMD_LAUNCH_CHECK(ctx, "group_reduce_kernel");
  }
  return PMD_OK;
}

}  // extern "C"
