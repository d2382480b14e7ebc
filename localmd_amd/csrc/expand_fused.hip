// Fused expansion of a decomposition into finished output frames (localmd_amd/export.py):
//   x[f][c] = mean[c] + std[c] * sum_g sum_k A_g[k][q_g(c)] * C[c_row0_g + k][f]
// with C = (R diag(s)) Vt[:, frames] (pmd_gemm) and A_g the dense blocks of U's columns that projection.py's group tables
// hold (tiles, and P_MAX-pixel chunks of the wide background columns).  It is the adjoint of pmd_group_project, and it
// replaces pmd_csr_rows_spmm + pmd_transpose_affine: no pixel-major accumulator, no transpose pass.  The epilogue also
// reads the raw frames in their own element type, forms the residual y - x, converts to the output type and writes
// every requested panel side by side into the frame-major output (T x d1 x P d2).
//
// One workgroup = one patch of 64 consecutive C-order pixels x one slab of 64 frames.  It walks the entries of its patch
// (one per group that touches the patch, in group order; export.py builds and validates them): each entry stages the
// group's C rows for the slab (Cs[k][f]) and the group's A columns for the patch's pixels (As[k][p], zero where a pixel
// is not in the group) into LDS, and the four waves contract them on v_mfma_f32_16x16x4_f32 (wave w: pixel tile w,
// all four frame tiles).  Both LDS arrays are k-major with a row stride of 80 floats: an operand read (lane i = l & 15,
// k = l >> 4) hits bank i + 16 k, conflict-free, and the staging writes are row-contiguous.
// Determinism: the sum of a pixel is one MFMA chain over the entries in table order and k ascending; the MFMA computes
// every frame column on its own, so frame f's bits do not depend on the call's frame offset or count.  No atomics.
#include "pmd_common.h"
#include "../../include/pmd_hip.h"
#include <type_traits>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int EX_PX = 64;    // pixels per workgroup (one patch)
constexpr int EX_FB = 64;    // frames per workgroup
constexpr int EX_KR = 64;    // rows per entry at most (MAX_ROWS of the group tables)
constexpr int EX_LS = 80;    // LDS row stride (floats)
constexpr int EX_OS = 65;    // row stride of the output staging (frames x pixels)
constexpr int EX_ET = 4;     // int64 fields per entry: {a_off, p64, r, c_row0}

template <typename E>
__device__ __forceinline__ float ex_load(const E* p) { return (float)*p; }

template <typename E, typename O>
__global__ __launch_bounds__(256) void group_expand_kernel(const float* __restrict__ C, long ldc, int n, long D, int d2,
                                                           const float* __restrict__ mean, const float* __restrict__ stdv,
                                                           const long* __restrict__ patch_ptr,
                                                           const long* __restrict__ entries, const int* __restrict__ qmap,
                                                           const float* __restrict__ A, const E* __restrict__ Y, long ldy,
                                                           int n_panels, int panels, O* __restrict__ out, long out_frame) {
  __shared__ float smem[2 * EX_KR * EX_LS];
  float* Cs = smem;                    // [k][frame]
  float* As = smem + EX_KR * EX_LS;    // [k][pixel]
  const long patch = blockIdx.x;
  const int f0 = blockIdx.y * EX_FB;
  const long c0 = patch * EX_PX;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const long e0 = patch_ptr[patch], e1 = patch_ptr[patch + 1];
  const int fl = min(f0 + lane, n - 1);   // staging column of this lane (clamped: loads stay inside C, masked below)
  const bool fv = f0 + lane < n;

  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (long e = e0; e < e1; ++e) {
    const long* et = entries + e * EX_ET;
    const long a_off = et[0], p64 = et[1], c_row0 = et[3];
    const int r = (int)et[2];
    const int r4 = (r + 3) & ~3;
    const int q = qmap[e * EX_PX + lane];
    const int qc = q < 0 ? 0 : q;
    // stage rows k = w, w + 4, ... < r4; rows in [r, r4) are zeros (A_g's padding rows are zero, C's are not ours)
    for (int k = w; k < r4; k += 4) {
      const bool kv = k < r;
      const int kc = kv ? k : 0;
      const float cv = C[(c_row0 + kc) * ldc + fl];
      const float av = A[a_off + (long)k * p64 + qc];
      Cs[k * EX_LS + lane] = (kv && fv) ? cv : 0.f;
      As[k * EX_LS + lane] = (kv && q >= 0) ? av : 0.f;
    }
    __syncthreads();
    const float* ap = As + lk * EX_LS + w * 16 + li;
    const float* bp = Cs + lk * EX_LS + li;
    for (int k = 0; k < r4; k += 4) {
      const float a = ap[k * EX_LS];
#pragma unroll
      for (int ft = 0; ft < 4; ++ft)
        acc[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[k * EX_LS + ft * 16], acc[ft], 0, 0, 0);
    }
    __syncthreads();
  }

  // D map of 16x16x4: column (frame) = lane & 15, rows (pixels) (lane >> 4) * 4 + v
  float* Os = smem;   // [frame][pixel]
#pragma unroll
  for (int ft = 0; ft < 4; ++ft)
#pragma unroll
    for (int v = 0; v < 4; ++v) Os[(ft * 16 + li) * EX_OS + w * 16 + lk * 4 + v] = acc[ft][v];
  __syncthreads();

  const long c = c0 + lane;
  if (c >= D) return;
  const float mu = mean[c], sg = stdv[c];
  const long i = c / d2, j = c - (c / d2) * d2;
  const long row_w = (long)n_panels * d2;
  O* ob = out + i * row_w + j;
  for (int f = w; f < EX_FB && f0 + f < n; f += 4) {
    const long fg = f0 + f;
    const float x = __fmaf_rn(sg, Os[f * EX_OS + lane], mu);
    float y = 0.f;
    if (Y) y = ex_load(Y + fg * ldy + c);
    O* o = ob + fg * out_frame;
    for (int p = 0; p < n_panels; ++p) {
      const int kind = (panels >> (2 * p)) & 3;
      const float v = kind == 0 ? y : (kind == 1 ? x : __fsub_rn(y, x));
      o[(long)p * d2] = pmd_quant<O>(v);
    }
  }
}

template <typename E, typename O>
void launch_expand(pmd_ctx* ctx, dim3 grid, const float* C, long ldc, int n, long D, int d2, const float* mean,
                   const float* std, const long* patch_ptr, const long* entries, const int* qmap, const float* A,
                   const void* Y, long ldy, int n_panels, int panels, void* out, long out_frame) {
  hipLaunchKernelGGL((group_expand_kernel<E, O>), grid, dim3(256), 0, ctx->stream, C, ldc, n, D, d2, mean, std, patch_ptr,
                     entries, qmap, A, (const E*)Y, ldy, n_panels, panels, (O*)out, out_frame);
}

}  // namespace

extern "C" {

int pmd_group_expand(pmd_ctx* ctx, const float* C, long ldc, int n, int d1, int d2, const float* mean, const float* std,
                     long n_patches, const long* patch_ptr, long n_entries, const long* entries, const int* qmap,
                     const float* A, const void* Y, int y_elem, long ldy, int n_panels, int panels, void* out,
                     int out_elem) {
  CTX_CHECK(ctx);
  const char* what = "pmd_group_expand";
  const long D = (long)d1 * d2;
  if (n < 0 || d1 < 1 || d2 < 1 || n_panels < 1 || n_panels > 3 || ldc < n || n_patches != (D + EX_PX - 1) / EX_PX)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (n >= 0, d1, d2 >= 1, 1..3 panels, ldc >= n, "
                                            "n_patches = ceil(D / 64))");
  if (pmd_bad_elem(y_elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown source element type");
  if (pmd_bad_elem(out_elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown output element type");
  bool needs_y = false;
  for (int p = 0; p < n_panels; ++p) {
    const int kind = (panels >> (2 * p)) & 3;
    if (kind > 2) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown panel code");
    needs_y |= kind != 1;
  }
  if (n == 0) return PMD_OK;
  if (n_entries < 0) return pmd_fail(ctx, PMD_ERR_ARG, what, "n_entries < 0");
  if (!mean || !std || !patch_ptr || !out || (needs_y && !Y) || (n_entries > 0 && (!C || !entries || !qmap || !A)))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if (needs_y && ldy < D) return pmd_fail(ctx, PMD_ERR_ARG, what, "ldy < d1 d2");
  const long n_fb = ((long)n + EX_FB - 1) / EX_FB;   // (in long: n + 63 overflows an int from 2^31 - 64 on)
  if (n_patches > 0x7fffffffL || n_fb > 65535) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many patches / frames in one call");
  pmd_prof_scope prof__(ctx, "group_expand");
  const dim3 grid((unsigned)n_patches, (unsigned)n_fb);
  const long out_frame = D * n_panels;
  const void* y = needs_y ? Y : nullptr;
  pmd_with_elem(y_elem, [&](auto e) {
    pmd_with_elem(out_elem, [&](auto o) {
      launch_expand<typename decltype(e)::type, typename decltype(o)::type>(
          ctx, grid, C, ldc, n, D, d2, mean, std, patch_ptr, entries, qmap, A, y, ldy, n_panels, panels, out, out_frame);
    });
  });
  PMD_LAUNCH_CHECK(ctx, "group_expand_kernel");
  return PMD_OK;
}

}  // extern "C"
