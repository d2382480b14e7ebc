// Exact per-pixel order statistics over time (localmd_amd/quantiles.py): a most-significant-digit-first radix select.
// Every element of a pixel is mapped to an order-preserving 32-bit key; a pass counts, per pixel, the 256 values of one
// 8-bit digit among the elements whose higher digits match the prefix found so far (pmd_pixel_hist_accumulate, once per
// batch), then picks the bin that holds the rank looked for (pmd_pixel_hist_select, once per pass).  After four passes
// the prefix is the key of the order statistic.  The device only counts integers: the result does not depend on how
// the frames are batched.
//
// Key of element y of pixel c: v = (float) y; with a centre, v = |v - centre[c]| (one fp32 subtraction, rounded to
// nearest, no contraction; the library is compiled with fp32 denormals kept, so a denormal difference is not flushed).
// key = ~bits(v) for bits with the sign set, bits(v) | 0x80000000 otherwise, and 0xFFFFFFFF for every NaN: unsigned key
// order is -inf < ... < -0 < +0 < ... < +inf < NaN.
//
// Histograms: hist is uint32 [ceil(D / 64)][256][64], indexed (pixel group, bin, pixel in group), so a wave that holds
// one pixel per lane reads and writes one bin of its group as 256 contiguous bytes.
//
// hist_kernel: a workgroup of four waves owns the 64 consecutive pixels of one group, lane l of every wave pixel
// 64 blockIdx + l (clamped to D - 1 for the loads of the last group; such a lane counts nothing).  The frames are cut
// into chunks of HQ_U; wave w takes chunks w, w + 4, ...: the HQ_U loads of its next chunk are issued, then the HQ_U
// increments of the chunk already in registers.  The counts go into a 64 KB LDS histogram [256][64] of dwords by LDS
// atomic adds without return (the four waves share the pixels); the LDS bank of an increment is its lane whatever the
// bin, so a wave's increments never conflict.  At the end the non-zero counters are added to hist by plain 16-byte loads
// and stores: the workgroup owns its pixels, no global atomics.  Two workgroups fit the 160 KB of LDS of a CU.
//
// select_kernel: a workgroup of four waves per group; wave w holds bins [64 w, 64 w + 64) of its lane's pixel in
// registers, the four quarter totals meet in LDS, and the wave whose quarter holds the rank scans it.  Every count read
// is set to zero for the next pass.
//
// Both launch nothing but their kernel: no synchronisation, no allocation, no workspace.
#include "pmd_common.h"
#include "../../include/pmd_hip.h"

namespace {

constexpr int HQ_WAVES = 4;
constexpr int HQ_U = 16;              // frames whose loads are in flight per lane
constexpr int HQ_BINS = 256;
constexpr int HQ_GROUP = 64;          // pixels per group = lanes of a wave

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned hq_key(float v) {
  const unsigned b = __float_as_uint(v);
  if (v != v) return 0xFFFFFFFFu;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <typename E>
__global__ __launch_bounds__(64 * HQ_WAVES) void hist_kernel(const E* __restrict__ Y, long ldy, long n, long D,
                                                              const float* __restrict__ centre, int pass,
                                                              const unsigned* __restrict__ prefix,
                                                              unsigned* __restrict__ hist) {
#pragma clang fp contract(off)
  __shared__ unsigned h[HQ_BINS * HQ_GROUP];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  u32x4* h4 = reinterpret_cast<u32x4*>(h);
  const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < HQ_BINS * HQ_GROUP / 4 / (64 * HQ_WAVES); ++i) h4[tid + i * 64 * HQ_WAVES] = zero;
  __syncthreads();

  const long c = (long)blockIdx.x * HQ_GROUP + lane;
  const bool live = c < D;
  const long cc = live ? c : D - 1;
  const bool centred = centre != nullptr;
  const float mu = centred ? centre[cc] : 0.f;
  const unsigned want = pass ? prefix[cc] : 0u;
  const int sh_hi = 32 - 8 * pass;    // pass > 0: key >> sh_hi is the prefix (sh_hi in 8 .. 24)
  const int sh_lo = 24 - 8 * pass;
  const E* col = Y + cc;

  E y[HQ_U], nx[HQ_U];
  auto load = [&](E* dst, long fs) {
#pragma unroll
    for (int u = 0; u < HQ_U; ++u) {
      const long f = fs + u < n ? fs + u : n - 1;   // past the end: re-read the last frame, not counted
      dst[u] = col[f * ldy];
    }
  };
  load(y, (long)w * HQ_U);
  for (long fs = (long)w * HQ_U; fs < n; fs += HQ_U * HQ_WAVES) {
    load(nx, fs + HQ_U * HQ_WAVES);                 // the next chunk's loads fly while this one is counted
#pragma unroll
    for (int u = 0; u < HQ_U; ++u) {
      float v = (float)y[u];
      if (centred) v = __builtin_fabsf(v - mu);
      const unsigned key = hq_key(v);
      const bool hit = live && fs + u < n && (pass == 0 || (key >> sh_hi) == want);
      if (hit)
        (void)__hip_atomic_fetch_add(&h[((key >> sh_lo) & 255u) * HQ_GROUP + lane], 1u, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_WORKGROUP);
    }
#pragma unroll
    for (int u = 0; u < HQ_U; ++u) y[u] = nx[u];
  }
  __syncthreads();

  u32x4* g4 = reinterpret_cast<u32x4*>(hist + (size_t)blockIdx.x * HQ_BINS * HQ_GROUP);
#pragma unroll 4
  for (int i = 0; i < HQ_BINS * HQ_GROUP / 4 / (64 * HQ_WAVES); ++i) {
    const int j = tid + i * 64 * HQ_WAVES;
    const u32x4 a = h4[j];
    if (a.x | a.y | a.z | a.w) g4[j] = g4[j] + a;
  }
}

__global__ __launch_bounds__(64 * HQ_WAVES) void select_kernel(long D, unsigned* __restrict__ hist, int* __restrict__ rank,
                                                                unsigned* __restrict__ prefix) {
  __shared__ unsigned tot[HQ_WAVES * HQ_GROUP];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr int Q = HQ_BINS / HQ_WAVES;             // bins per wave
  unsigned* g = hist + (size_t)blockIdx.x * HQ_BINS * HQ_GROUP + (size_t)w * Q * HQ_GROUP + lane;
  unsigned cnt[Q];
  unsigned sum = 0;
#pragma unroll
  for (int b = 0; b < Q; ++b) {
    cnt[b] = g[b * HQ_GROUP];
    sum += cnt[b];
  }
#pragma unroll
  for (int b = 0; b < Q; ++b) g[b * HQ_GROUP] = 0u;
  tot[w * HQ_GROUP + lane] = sum;
  __syncthreads();
  const long c = (long)blockIdx.x * HQ_GROUP + lane;
  if (c >= D) return;
  unsigned below = 0;
  for (int s = 0; s < w; ++s) below += tot[s * HQ_GROUP + lane];
  const unsigned r = (unsigned)rank[c];
  if (r < below || r >= below + sum) return;         // the rank lies in another wave's quarter (or beyond the count)
  int bin = 0;
  unsigned under = below;                            // the count below the bin that holds the rank
  bool found = false;
#pragma unroll
  for (int b = 0; b < Q; ++b) {
    if (!found) {
      if (r < under + cnt[b]) {
        found = true;
        bin = b;
      } else {
        under += cnt[b];
      }
    }
  }
  rank[c] = (int)(r - under);
  prefix[c] = (prefix[c] << 8) | (unsigned)(w * Q + bin);
}

}  // namespace

extern "C" {

int pmd_pixel_hist_accumulate(pmd_ctx* ctx, const void* Y, int elem, long ldy, long n, long D, const float* centre,
                              int pass, const uint32_t* prefix, uint32_t* hist) {
  CTX_CHECK(ctx);
  const char* what = "pmd_pixel_hist_accumulate";
  if (n < 1 || n >= 0x80000000L) return pmd_fail(ctx, PMD_ERR_ARG, what, "n outside 1 .. 2^31 - 1");
  if (D < 1 || ldy < D) return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (D >= 1, ldy >= D)");
  if (pass < 0 || pass > 3) return pmd_fail(ctx, PMD_ERR_ARG, what, "pass outside 0 .. 3");
  if (pmd_bad_elem(elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown element type");
  if (!Y || !hist) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if (pass > 0 && !prefix) return pmd_fail(ctx, PMD_ERR_ARG, what, "a pass after the first needs prefix");
  if ((uintptr_t)hist % 16 != 0) return pmd_fail(ctx, PMD_ERR_ARG, what, "hist is not 16-byte aligned");
  if ((D + HQ_GROUP - 1) / HQ_GROUP > 0x7fffffffL) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many pixels in one call");
  pmd_prof_scope prof__(ctx, "pixel_hist_accumulate");
  const dim3 grid((unsigned)((D + HQ_GROUP - 1) / HQ_GROUP)), block(64 * HQ_WAVES);
  pmd_with_elem(elem, [&](auto e) {
    using E = typename decltype(e)::type;
    hipLaunchKernelGGL(hist_kernel<E>, grid, block, 0, ctx->stream, (const E*)Y, ldy, n, D, centre, pass, prefix, hist);
  });
  PMD_LAUNCH_CHECK(ctx, "hist_kernel");
  return PMD_OK;
}

int pmd_pixel_hist_select(pmd_ctx* ctx, long D, uint32_t* hist, int* rank, uint32_t* prefix) {
  CTX_CHECK(ctx);
  const char* what = "pmd_pixel_hist_select";
  if (D < 1) return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (D >= 1)");
  if (!hist || !rank || !prefix) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if ((D + HQ_GROUP - 1) / HQ_GROUP > 0x7fffffffL) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many pixels in one call");
  pmd_prof_scope prof__(ctx, "pixel_hist_select");
  const dim3 grid((unsigned)((D + HQ_GROUP - 1) / HQ_GROUP)), block(64 * HQ_WAVES);
  hipLaunchKernelGGL(select_kernel, grid, block, 0, ctx->stream, D, hist, rank, prefix);
  PMD_LAUNCH_CHECK(ctx, "select_kernel");
  return PMD_OK;
}

}  // extern "C"
