// Separable spatial filtering of a movie's frames (localmd_amd/spatial.py): out = centre a + (wy x wx) * a - box (1 x 1) * a
// with reflected borders, the Gaussian low-pass, Gaussian-minus-window-mean band-pass and identity-minus-Gaussian
// high-pass of one-photon preprocessing (pmd_spatial_filter).
//
// filter_kernel       a workgroup of 256 threads takes one frame and one SF_TH x SF_TW tile of it.
//   row pass          for the tile's rows and ry halo rows above and below (reflected into the frame), thread (row, x)
//                     walks the 2 rx + 1 taps of source row refl(y) with x reflected per tap: the loads of a wave are 64
//                     consecutive elements (two runs at a reflected border), served by the vector cache after the first
//                     tap, and widened to fp32 in registers.  A tile none of whose taps leaves the frame (all but the
//                     first and last tile of a row) skips the reflection: its taps are consecutive elements behind one
//                     pointer, which takes the index arithmetic, not the loads, out of the inner loop.  h (the weighted
//                     chain) and, for a band-pass, s (the plain add chain) go to two LDS planes of (SF_TH + 2 ry) x
//                     SF_TW floats.  A plane row is 64 floats: the lanes of a wave write and read consecutive banks, so
//                     neither pass has a bank conflict.
//   column pass       thread (row, x) walks the 2 ry + 1 plane rows of its column in LDS, adds the centre term and
//                     subtracts the box term, quantises and stores: 64 consecutive elements per wave.
//                     The tile is not staged: at radius 32 a staged tile and two planes do not fit 64 KB of LDS, the
//                     planes alone (48 KB) do, and one layout serves every radius.
// The weights travel by value in the kernel's arguments (two arrays of 65 floats, read with scalar loads: the tap index is
// the same for the whole wave), so the call has no device table, no workspace and no synchronisation.
// Every product and every sum is rounded on its own (contraction is off) and every chain runs over ascending taps, so the
// bits of a pixel depend on the frame, the weights and the geometry only.
#include "pmd_common.h"
#include "../../include/pmd_hip.h"

namespace {

constexpr int SF_TH = 32;            // rows of a tile
constexpr int SF_TW = 64;            // columns of a tile: one wave per plane row
constexpr int SF_THREADS = 256;
constexpr int SF_TAPS = 2 * PMD_FILTER_MAX_RADIUS + 1;

struct sf_weights {
  float wy[SF_TAPS], wx[SF_TAPS];
};

__device__ __forceinline__ int sf_refl(int i, int d) { return i < 0 ? -1 - i : (i >= d ? 2 * d - 1 - i : i); }

template <typename E, typename O, bool BOX>
__global__ __launch_bounds__(SF_THREADS) void filter_kernel(const E* __restrict__ X, long fs, long rs, int d1, int d2,
                                                             int ry, int rx, const sf_weights w, float centre, float box,
                                                             int tiles_x, O* __restrict__ out, long ofs, long ors) {
#pragma clang fp contract(off)
  extern __shared__ float sf_lds[];
  const int tile = (int)blockIdx.x, ty0 = (tile / tiles_x) * SF_TH, tx0 = (tile % tiles_x) * SF_TW;
  const int tx = (int)threadIdx.x & (SF_TW - 1), r0 = (int)threadIdx.x / SF_TW;
  const int th = min(SF_TH, d1 - ty0), rows = th + 2 * ry, x = tx0 + tx;
  const E* F = X + (long)blockIdx.y * fs;
  float* H = sf_lds;
  float* S = sf_lds + (SF_TH + 2 * ry) * SF_TW;
  // no tap of this tile's columns leaves the frame (the same for the whole workgroup): the taps are consecutive elements
  const bool inside = tx0 >= rx && tx0 + SF_TW - 1 + rx < d2;
  if (x < d2) {
    for (int k = r0; k < rows; k += SF_THREADS / SF_TW) {
      const E* row = F + (long)sf_refl(ty0 - ry + k, d1) * rs;
      float acc, sum;
      if (inside) {
        const E* p = row + (x - rx);
        const float a0 = (float)p[0];
        acc = w.wx[0] * a0, sum = a0;
#pragma unroll 4
        for (int j = 1; j <= 2 * rx; ++j) {
          const float a = (float)p[j];
          acc = acc + w.wx[j] * a;
          if (BOX) sum = sum + a;
        }
      } else {
        const float a0 = (float)row[sf_refl(x - rx, d2)];
        acc = w.wx[0] * a0, sum = a0;
        for (int j = 1; j <= 2 * rx; ++j) {
          const float a = (float)row[sf_refl(x + j - rx, d2)];
          acc = acc + w.wx[j] * a;
          if (BOX) sum = sum + a;
        }
      }
      H[k * SF_TW + tx] = acc;
      if (BOX) S[k * SF_TW + tx] = sum;
    }
  }
  __syncthreads();
  if (x >= d2) return;
  for (int k = r0; k < th; k += SF_THREADS / SF_TW) {
    const float* hp = H + k * SF_TW + tx;
    const float* sp = S + k * SF_TW + tx;
    float g = w.wy[0] * hp[0], sum = BOX ? sp[0] : 0.f;
#pragma unroll 4
    for (int i = 1; i <= 2 * ry; ++i) {
      g = g + w.wy[i] * hp[i * SF_TW];
      if (BOX) sum = sum + sp[i * SF_TW];
    }
    const long y = ty0 + k;
    float v = g;
    if (centre != 0.f) v = centre * (float)F[y * rs + x] + g;
    if (BOX) v = v - box * sum;
    out[(long)blockIdx.y * ofs + y * ors + x] = pmd_quant<O>(v);
  }
}

template <typename E, typename O>
void launch_filter(pmd_ctx* ctx, const void* X, long fs, long rs, int n0, int g, int d1, int d2, int ry, int rx,
                   const sf_weights& w, float centre, float box, void* out, long ofs, long ors) {
  const int tiles_x = (d2 + SF_TW - 1) / SF_TW, tiles_y = (d1 + SF_TH - 1) / SF_TH;
  const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)g);
  const size_t plane = (size_t)(SF_TH + 2 * ry) * SF_TW * sizeof(float);
  const E* x = (const E*)X + (long)n0 * fs;
  O* o = (O*)out + (long)n0 * ofs;
  if (box != 0.f)
    hipLaunchKernelGGL((filter_kernel<E, O, true>), grid, dim3(SF_THREADS), 2 * plane, ctx->stream, x, fs, rs, d1, d2, ry, rx,
                       w, centre, box, tiles_x, o, ofs, ors);
  else
    hipLaunchKernelGGL((filter_kernel<E, O, false>), grid, dim3(SF_THREADS), plane, ctx->stream, x, fs, rs, d1, d2, ry, rx, w,
                       centre, box, tiles_x, o, ofs, ors);
}

}  // namespace

extern "C" {

int pmd_spatial_filter(pmd_ctx* ctx, const void* X, int elem, long frame_stride, long row_stride, int n, int d1, int d2,
                       int ry, int rx, const float* wy_host, const float* wx_host, float centre, float box, void* out,
                       int out_elem, long out_frame_stride, long out_row_stride) {
  CTX_CHECK(ctx);
  const char* what = "pmd_spatial_filter";
  if (n < 0) return pmd_fail(ctx, PMD_ERR_ARG, what, "n is negative");
  if (d1 < 1 || d2 < 1 || d1 > PMD_SHIFT_MAX_DIM || d2 > PMD_SHIFT_MAX_DIM)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "frame sides outside 1 .. 16384");
  if (ry < 0 || rx < 0 || ry > PMD_FILTER_MAX_RADIUS || rx > PMD_FILTER_MAX_RADIUS || ry > d1 || rx > d2)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "a radius outside 0 .. min(32, the frame's side)");
  if (pmd_bad_elem(elem) || pmd_bad_elem(out_elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown element type");
  if (pmd_short_strides(frame_stride, row_stride, d1, d2) ||
      pmd_short_strides(out_frame_stride, out_row_stride, d1, d2))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "a stride is shorter than a row / a frame");
  if (!X || !wy_host || !wx_host || !out) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if (n == 0) return PMD_OK;
  if (pmd_images_overlap(X, elem, frame_stride, row_stride, out, out_elem, out_frame_stride, out_row_stride, n, d1, d2))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "X and out overlap");
  sf_weights w;
  for (int i = 0; i < SF_TAPS; ++i) {
    w.wy[i] = i <= 2 * ry ? wy_host[i] : 0.f;
    w.wx[i] = i <= 2 * rx ? wx_host[i] : 0.f;
  }
  pmd_prof_scope prof__(ctx, "spatial_filter");
  for (int n0 = 0; n0 < n; n0 += 32768) {
    const int g = n - n0 < 32768 ? n - n0 : 32768;
    pmd_with_elem(elem, [&](auto e) {
      pmd_with_elem(out_elem, [&](auto o) {
        launch_filter<typename decltype(e)::type, typename decltype(o)::type>(
            ctx, X, frame_stride, row_stride, n0, g, d1, d2, ry, rx, w, centre, box, out, out_frame_stride, out_row_stride);
      });
    });
    PMD_LAUNCH_CHECK(ctx, "filter_kernel");
  }
  return PMD_OK;
}

}  // extern "C"
