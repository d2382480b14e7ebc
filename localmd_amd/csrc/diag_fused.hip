// One-pass fit diagnostics of a decomposition against its movie (localmd_amd.diagnostic_images.make_pmd_diagnostic_images):
// the moments behind the four images of the reference's localmd/diagnostic_plots.py (make_correlation_image,
// make_autocorrelation_image, make_pmd_correlation_image, make_residual_correlation_image) plus the residual statistics,
// from ONE read of the movie.  Per frame t and pixel p, with y the raw frame (source dtype, converted to fp32), w the
// reconstruction std * (U R s Vt) without its mean (frames-first fp32, built by pmd_gemm + the expansion kernels) and
// r = (y - mean) - w the residual (never the difference of two values of the order of the mean):
//   moments[ 0..10)[p]  neighbour moments of y      (layout of pmd_neighbour_moments: sum x, sum x^2, sum x_p x_q)
//   moments[10..20)[p]  neighbour moments of w
//   moments[20..30)[p]  neighbour moments of r
//   moments[30..35)[p]  lag moments of y            (layout of pmd_lag_moments, pairs (t, t - lag), t >= lag)
//   frame_ss[t]         sum over the pixels of r_t^2 (unshifted)
// Numerics of diag.hip: every trace is shifted by its value in frame 0 (ref[3][D], written by this call when it holds
// frame 0), products are summed in fp32 over slices of at most 64 frames, everything above that in fp64.
//
// Reduction tree: slices are the absolute frame ranges [64 k, 64 k + 64); a workgroup owns the absolute frame block
// [DF_FPB b, DF_FPB b + DF_FPB) and adds its slices in order; the blocks are added to the running moments in order of b
// (reduce_kernel).  A call must start on a block boundary, so the tree depends on absolute frame indices only, never on
// how the frames were batched.  frame_ss[t] is a fixed-order wave sum (xor butterfly), four waves in order, then the pixel
// blocks in order - no atomics anywhere.
// Lag pairs whose earlier frame lies before the batch read it from a ring of `lag` raw frames (slot = frame mod lag) that
// the caller fills after each batch.
#include "pmd_common.h"
#include "../../include/pmd_hip.h"

namespace {

constexpr int DF_SLICE = 64;   // frames whose products are summed in fp32
constexpr int DF_FPB = 512;    // frames per workgroup: the fp64 partial of one absolute frame block
constexpr int DF_NM = 35;      // moments per pixel

template <typename E>
__device__ __forceinline__ float ld_f(const E* p, long i) { return (float)p[i]; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// ref[0][p] = y_0, ref[1][p] = w_0, ref[2][p] = (y_0 - mean) - w_0
template <typename E>
__global__ __launch_bounds__(256) void ref_kernel(const E* __restrict__ Y, const float* __restrict__ W,
                                                  const float* __restrict__ mean, long D, float* __restrict__ ref) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= D) return;
  const float y = ld_f(Y, p), w = W[p];
  ref[p] = y;
  ref[D + p] = w;
  ref[2 * D + p] = (y - mean[p]) - w;
}

// partial[blk][35][D] for the frame blocks of frames [c0, c0 + n); pss[pixel block][n] = per-frame residual sums
template <typename E>
__global__ __launch_bounds__(256) void fused_kernel(const E* __restrict__ Y, long ybase, const float* __restrict__ W,
                                                    const E* __restrict__ ring, int lag, long c0, int n, int d1, int d2,
                                                    const float* __restrict__ mean, const float* __restrict__ ref,
                                                    double* __restrict__ partial, double* __restrict__ pss) {
  __shared__ float red[4][DF_SLICE];
  const long D = (long)d1 * d2;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  const bool ok = p < D;
  const long pc = ok ? p : D - 1;
  const int i = (int)(pc / d2), j = (int)(pc - (long)i * d2);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int q[8];
  float ry[8], rw[8], rr[8], mq[8];
  int k = 0;
#pragma unroll
  for (int di = -1; di <= 1; ++di)
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj) {
      if (di == 0 && dj == 0) continue;
      const int ii = min(max(i + di, 0), d1 - 1), jj = min(max(j + dj, 0), d2 - 1);  // clamped: the image step ignores them
      q[k] = ii * d2 + jj;
      ry[k] = ref[q[k]];
      rw[k] = ref[D + q[k]];
      rr[k] = ref[2 * D + q[k]];
      mq[k] = mean[q[k]];
      ++k;
    }
  const float ryp = ref[pc], rwp = ref[D + pc], rrp = ref[2 * D + pc], mp = mean[pc];
  double acc[DF_NM];
#pragma unroll
  for (int m = 0; m < DF_NM; ++m) acc[m] = 0.0;
  const long t0 = c0 + (long)blockIdx.y * DF_FPB;            // absolute frames [t0, t1)
  const long t1 = min(c0 + n, t0 + DF_FPB);
  const long lag0 = lag;
  for (long ts = t0; ts < t1; ts += DF_SLICE) {
    float f[DF_NM];
#pragma unroll
    for (int m = 0; m < DF_NM; ++m) f[m] = 0.f;
    const long te = min(t1, ts + DF_SLICE);
    for (long t = ts; t < te; ++t) {
      const E* y = Y + (t - ybase) * D;
      const float* w = W + (t - c0) * D;
      const float yp = ld_f(y, pc), wp = w[pc];
      const float rp = (yp - mp) - wp;
      const float xp = yp - ryp, vp = wp - rwp, sp = rp - rrp;
      f[0] += xp; f[1] += xp * xp;
      f[10] += vp; f[11] += vp * vp;
      f[20] += sp; f[21] += sp * sp;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const float yq = ld_f(y, q[m]), wq = w[q[m]];
        f[2 + m] += xp * (yq - ry[m]);
        f[12 + m] += vp * (wq - rw[m]);
        f[22 + m] += sp * (((yq - mq[m]) - wq) - rr[m]);
      }
      if (t >= lag0) {
        const long tl = t - lag0;
        const float yl = (tl >= ybase ? ld_f(Y + (tl - ybase) * D, pc) : ld_f(ring + (tl % lag0) * D, pc)) - ryp;
        f[30] += xp; f[31] += xp * xp; f[32] += yl; f[33] += yl * yl; f[34] += xp * yl;
      }
      const float s = wave_sum(ok ? rp * rp : 0.f);
      if (lane == 0) red[wv][t - ts] = s;
    }
#pragma unroll
    for (int m = 0; m < DF_NM; ++m) acc[m] += (double)f[m];
    __syncthreads();
    if (threadIdx.x < te - ts) {
      const int u = threadIdx.x;
      pss[(long)blockIdx.x * n + (ts - c0) + u] = (((double)red[0][u] + (double)red[1][u]) + (double)red[2][u]) + (double)red[3][u];
    }
    __syncthreads();
  }
  if (!ok) return;
  double* o = partial + (long)blockIdx.y * DF_NM * D + p;
#pragma unroll
  for (int m = 0; m < DF_NM; ++m) o[(long)m * D] = acc[m];
}

// moments[e] += partial[0][e] + partial[1][e] + ... (in block order), e < 35 D
__global__ void reduce_kernel(const double* __restrict__ partial, long n_elems, int blocks, double* __restrict__ moments) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_elems) return;
  double s = moments[e];
  for (int b = 0; b < blocks; ++b) s += partial[(long)b * n_elems + e];
  moments[e] = s;
}

// frame_ss[c0 + t] = sum over the pixel blocks of pss[pb][t] (in block order)
__global__ void frame_ss_kernel(const double* __restrict__ pss, int n, int n_pb, long c0, double* __restrict__ frame_ss) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  double s = 0.0;
  for (int b = 0; b < n_pb; ++b) s += pss[(long)b * n + t];
  frame_ss[c0 + t] = s;
}

template <typename E>
int launch(pmd_ctx* ctx, const E* Y, long ybase, const float* W, const E* ring, int lag, long c0, int n, int d1, int d2,
           const float* mean, float* ref, double* moments, double* frame_ss, double* partial, double* pss) {
  const long D = (long)d1 * d2;
  const unsigned gx = (unsigned)((D + 255) / 256);
  if (c0 == 0) {
    hipLaunchKernelGGL(ref_kernel<E>, dim3(gx), dim3(256), 0, ctx->stream, Y + (0 - ybase) * D, W, mean, D, ref);
    PMD_LAUNCH_CHECK(ctx, "diag_ref_kernel");
  }
  const int blocks = (n + DF_FPB - 1) / DF_FPB;
  hipLaunchKernelGGL(fused_kernel<E>, dim3(gx, (unsigned)blocks), dim3(256), 0, ctx->stream, Y, ybase, W, ring, lag, c0, n,
                     d1, d2, mean, ref, partial, pss);
  PMD_LAUNCH_CHECK(ctx, "diag_fused_kernel");
  hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)((DF_NM * D + 255) / 256)), dim3(256), 0, ctx->stream, partial, DF_NM * D,
                     blocks, moments);
  PMD_LAUNCH_CHECK(ctx, "diag_reduce_kernel");
  hipLaunchKernelGGL(frame_ss_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, pss, n, (int)gx, c0,
                     frame_ss);
  PMD_LAUNCH_CHECK(ctx, "diag_frame_ss_kernel");
  return PMD_OK;
}

}  // namespace

extern "C" {

size_t pmd_diag_fused_workspace_bytes(int n, long D) {
  if (n <= 0 || D <= 0) return 0;
  const long blocks = (n + DF_FPB - 1) / DF_FPB;
  const long pixel_blocks = (D + 255) / 256;
  return (size_t)blocks * DF_NM * (size_t)D * sizeof(double) + (size_t)pixel_blocks * (size_t)n * sizeof(double);
}

int pmd_diag_fused_accumulate(pmd_ctx* ctx, const void* Y, int elem, long ybase, const float* W, const void* ring, int lag,
                              long c0, int n, long T, int d1, int d2, const float* mean, float* ref, double* moments,
                              double* frame_ss, void* ws, size_t ws_bytes) {
  CTX_CHECK(ctx);
  const char* what = "pmd_diag_fused_accumulate";
  if (pmd_bad_elem(elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown element type");
  if (d1 < 1 || d2 < 1 || (long)d1 * d2 > 0x7fffffffL || T < 2 || lag < 1 || lag >= T)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "bad shape (d1, d2 >= 1, d1 d2 < 2^31, T >= 2, 1 <= lag < T)");
  if (n < 1 || c0 < 0 || c0 % DF_FPB != 0 || c0 + n > T || ybase < 0 || ybase > c0)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "frames: need n >= 1, c0 a multiple of 512, c0 + n <= T, 0 <= ybase <= c0");
  if (c0 == 0 && ybase != 0) return pmd_fail(ctx, PMD_ERR_ARG, what, "the call holding frame 0 needs ybase = 0");
  if (!Y || !W || !mean || !ref || !moments || !frame_ss || !ws) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  // the earliest pair (max(c0, lag), max(c0, lag) - lag) reaches before the batch
  if (c0 + n - 1 >= lag && (c0 > lag ? c0 : (long)lag) - lag < ybase && !ring)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "lag pairs reach before the batch: a ring of lag frames is needed");
  if (ws_bytes < pmd_diag_fused_workspace_bytes(n, (long)d1 * d2)) return pmd_fail(ctx, PMD_ERR_WORKSPACE, what, "workspace too small");
  pmd_prof_scope prof__(ctx, "diag_fused");
  const long D = (long)d1 * d2;
  const long blocks = (n + DF_FPB - 1) / DF_FPB;
  double* partial = (double*)ws;
  double* pss = partial + blocks * DF_NM * D;
  int rc = PMD_OK;
  pmd_with_elem(elem, [&](auto e) {
    using E = typename decltype(e)::type;
    rc = launch<E>(ctx, (const E*)Y, ybase, W, (const E*)ring, lag, c0, n, d1, d2, mean, ref, moments, frame_ss, partial, pss);
  });
  return rc;
}

}  // extern "C"
