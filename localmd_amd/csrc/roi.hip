// Raw ROI traces (localmd_amd/traces.py):  out[k][f] = sum_q w[q] * (float) Y[f][pix[q]]  over the pixels of ROI k, for a
// frames-first batch Y (n x D; float32 / uint16 / int16 converted in the kernel).  The tables (traces.roi_tables) list
// every ROI's pixels as C-order ids in ascending order, so the 64 lanes of a wave read runs of consecutive addresses
// whatever the decomposition's pixel order is, and cut an ROI longer than ROI_SEG pixels into segments, so that a
// whole-field mask fills the machine like a thousand cell masks do.
//
// One workgroup = one segment x one block of 64 frames; wave w owns the frames f0 + 16 w .. f0 + 16 w + 15.  The
// segment's pixels are walked in chunks of 64: lane l loads pix / w of pixel q + l once per chunk, issues the 16 loads
// of its frames (unconditional, on clamped indices; masked afterwards) and then the 16 fmas into 16 private
// accumulators that live across all chunks.  Only after the last chunk one xor butterfly per frame (1, 2, ..., 32)
// folds the 64 lanes.  No LDS, no atomics, no cross-lane traffic inside the loop.
// The sum of out[k][f] is therefore: per lane the fma chain over its pixels q = l, l + 64, ... from 0, the butterfly,
// and for a split ROI the partial sums of its segments added in segment order by roi_reduce_kernel - an order fixed by
// the tables alone: it depends neither on n, nor on the frame's position in the batch, nor on the element type.
//
// Grid: workgroup id = segment * n_frame_blocks + frame block, so the frame blocks of a segment (which share its pixel
// and weight lists) are neighbours in the launch order.
#include "pmd_common.h"
#include "../../include/pmd_hip.h"

namespace {

constexpr int RG_FB = 64;    // frames per workgroup
constexpr int RG_FW = 16;    // frames per wave (private accumulators per lane)
constexpr int RG_ST = 4;     // int64 entries per segment: {q0, p, out_row, to_ws}

// Lane exchange of the butterfly.  Steps 1 and 2 are quad permutes and steps 4 and 8 the half-row / row mirrors of DPP:
// after steps 1 and 2 the four lanes of a quad hold the same bits (a + b and b + a are the same fp32), so the mirror
// partner 7 - i (15 - i) holds what lane i ^ 4 (i ^ 8) holds.  Step 16 is a ds_swizzle in bit mode (and 0x1f, xor 0x10),
// step 32 the one exchange that needs the full crossbar.
template <int CTRL>
__device__ __forceinline__ float dpp_get(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// Sum over the 64 lanes, left in every lane: v += partner(v) for the steps 1, 2, 4, 8, 16, 32 in this order.
__device__ __forceinline__ float fold64(float v) {
  v += dpp_get<0xB1>(v);     // quad_perm [1, 0, 3, 2]
  v += dpp_get<0x4E>(v);     // quad_perm [2, 3, 0, 1]
  v += dpp_get<0x141>(v);    // row_half_mirror
  v += dpp_get<0x140>(v);    // row_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F));
  v += __shfl_xor(v, 32, 64);
  return v;
}

template <typename E>
__global__ __launch_bounds__(256) void roi_gather_kernel(const E* __restrict__ Y, int n, long D,
                                                         const long* __restrict__ segs, int n_fb,
                                                         const int* __restrict__ pix, const float* __restrict__ wt,
                                                         float* __restrict__ out, long ldo, float* __restrict__ ws) {
  const long s = (long)blockIdx.x / n_fb;
  const int f0 = (int)((long)blockIdx.x - s * n_fb) * RG_FB;
  const long* st = segs + s * RG_ST;
  const long q0 = st[0], out_row = st[2];
  const int p = (int)st[1], to_ws = (int)st[3];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int fw = f0 + RG_FW * w;                 // first frame of this wave
  if (fw >= n) return;                           // wave-uniform: no frame of this wave exists
  const E* yrow[RG_FW];                          // wave-uniform row bases (frames beyond n read frame n - 1)
#pragma unroll
  for (int u = 0; u < RG_FW; ++u) yrow[u] = Y + (long)min(fw + u, n - 1) * D;
  float acc[RG_FW];
#pragma unroll
  for (int u = 0; u < RG_FW; ++u) acc[u] = 0.f;

  for (int q = 0; q < p; q += 64) {
    const int ql = q + lane;
    const bool qv = ql < p;
    const long qi = q0 + (qv ? ql : 0);          // idle lanes of the last chunk re-read the segment's first pixel
    const long c = pix[qi];
    const float wv = wt[qi];
    float y[RG_FW];
#pragma unroll
    for (int u = 0; u < RG_FW; ++u) y[u] = (float)yrow[u][c];
#pragma unroll
    for (int u = 0; u < RG_FW; ++u) acc[u] = qv ? __builtin_fmaf(wv, y[u], acc[u]) : acc[u];
  }

  float mine = 0.f;                              // lane u < 16 keeps the folded sum of frame fw + u
#pragma unroll
  for (int u = 0; u < RG_FW; ++u) {
    const float v = fold64(acc[u]);
    if (lane == u) mine = v;
  }
  float* dst = to_ws ? ws : out;
  const long ld = to_ws ? (long)n : ldo;
  if (lane < RG_FW && fw + lane < n) dst[out_row * ld + fw + lane] = mine;
}

// out[out_row][f] = sum_{c < parts} ws[ws_row0 + c][f], c ascending from 0.f.
__global__ __launch_bounds__(256) void roi_reduce_kernel(const long* __restrict__ split, int n,
                                                         const float* __restrict__ ws, float* __restrict__ out, long ldo) {
  const long* t = split + (long)blockIdx.y * 3;
  const long out_row = t[0], row0 = t[1];
  const int parts = (int)t[2];
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n) return;
  float s = 0.f;
  for (int c = 0; c < parts; ++c) s += ws[(row0 + c) * n + f];
  out[out_row * ldo + f] = s;
}

// d = C[k][f] + offset[k] (C == NULL: offset alone); den[k][f] = d; res[k][f] = raw[k][f] - d (from the rounded d).
__global__ __launch_bounds__(256) void roi_combine_kernel(int K, int n, const float* __restrict__ C, long ldc,
                                                          const float* __restrict__ offset,
                                                          const float* __restrict__ raw, long ldr,
                                                          float* __restrict__ den, long ldd, float* __restrict__ res,
                                                          long lde) {
  const long k = blockIdx.y;
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n) return;
  const float o = offset[k];
  const float d = C ? C[k * ldc + f] + o : o;
  if (den) den[k * ldd + f] = d;
  if (res) res[k * lde + f] = raw[k * ldr + f] - d;
}

}  // namespace

extern "C" {

size_t pmd_roi_gather_workspace_bytes(long n_partial_rows, int n) {
  if (n_partial_rows <= 0 || n <= 0) return 0;
  return (size_t)n_partial_rows * (size_t)n * sizeof(float);
}

int pmd_roi_gather(pmd_ctx* ctx, const void* Y, int elem, int n, long D, long n_segs, const long* segs, const int* pix,
                   const float* w, long n_partial_rows, int n_split, const long* split, float* out, long ldo, void* ws,
                   size_t ws_bytes) {
  CTX_CHECK(ctx);
  const char* what = "pmd_roi_gather";
  if (n < 0 || D < 1 || n_segs < 0 || n_split < 0 || n_partial_rows < 0 || ldo < n)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (n >= 0, D >= 1, counts >= 0, ldo >= n)");
  if (pmd_bad_elem(elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown element type");
  if ((n_split > 0) != (n_partial_rows > 0))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "partial rows and split ROIs come together");
  if (n == 0 || n_segs == 0) return PMD_OK;
  if (!Y || !segs || !pix || !w || !out || (n_split > 0 && !split)) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if (ws_bytes < pmd_roi_gather_workspace_bytes(n_partial_rows, n) || (n_partial_rows > 0 && !ws))
    return pmd_fail(ctx, PMD_ERR_WORKSPACE, what, "workspace too small");
  const long n_fb = ((long)n + RG_FB - 1) / RG_FB;   // (in long: n + 63 overflows an int from 2^31 - 64 on)
  if (n_segs * n_fb > 0x7fffffffL) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many segments x frame blocks");
  pmd_prof_scope prof__(ctx, "roi_gather");
  const dim3 grid((unsigned)(n_segs * n_fb));
  float* wsf = (float*)ws;
  pmd_with_elem(elem, [&](auto e) {
    using E = typename decltype(e)::type;
    hipLaunchKernelGGL(roi_gather_kernel<E>, grid, dim3(256), 0, ctx->stream, (const E*)Y, n, D, segs, (int)n_fb, pix, w,
                       out, ldo, wsf);
  });
  PMD_LAUNCH_CHECK(ctx, "roi_gather_kernel");
  if (n_split > 0) {
    for (int r0 = 0; r0 < n_split; r0 += 65535) {
      const int rn = (n_split - r0 < 65535) ? n_split - r0 : 65535;
      hipLaunchKernelGGL(roi_reduce_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)rn), dim3(256), 0, ctx->stream,
                         split + (long)r0 * 3, n, wsf, out, ldo);
    }
    PMD_LAUNCH_CHECK(ctx, "roi_reduce_kernel");
  }
  return PMD_OK;
}

int pmd_roi_combine(pmd_ctx* ctx, long K, int n, const float* C, long ldc, const float* offset, const float* raw, long ldr,
                    float* den, long ldd, float* res, long lde) {
  CTX_CHECK(ctx);
  const char* what = "pmd_roi_combine";
  if (K < 0 || n < 0 || (C && ldc < n) || (den && ldd < n) || (res && (lde < n || ldr < n)))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (K, n >= 0, leading dimensions >= n)");
  if (K == 0 || n == 0 || (!den && !res)) return PMD_OK;
  if (!offset || (res && !raw)) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  pmd_prof_scope prof__(ctx, "roi_combine");
  for (long k0 = 0; k0 < K; k0 += 65535) {
    const long kn = (K - k0 < 65535) ? K - k0 : 65535;
    hipLaunchKernelGGL(roi_combine_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)kn), dim3(256), 0, ctx->stream,
                       (int)kn, n, C ? C + k0 * ldc : nullptr, ldc, offset + k0, raw ? raw + k0 * ldr : nullptr, ldr,
                       den ? den + k0 * ldd : nullptr, ldd, res ? res + k0 * lde : nullptr, lde);
  }
  PMD_LAUNCH_CHECK(ctx, "roi_combine_kernel");
  return PMD_OK;
}

}  // extern "C"
