// Growing ROI supports (localmd_amd/grow.py): the moments of every (pixel, ROI) pair of every ROI's window against the
// ROI's trace, on the movie with the other ROIs of that pixel taken out.
//
// pmd_roi_window_moments_accumulate.  Pair i is pixel pair_px[i] and ROI pair_k[i]; its others are the entries q of
// [oth_ptr[i], oth_ptr[i + 1]): the ROIs other than pair_k[i] with a non-zero footprint value oth_a[q] on that pixel.  Per
// frame f: y = (float) X[f][px]; for q in stored order y = fl32(y - fl32(oth_a[q] * Ct[f][oth_k[q]])); c = Ct[f][k]; three
// fp64 sums per pair over the frames: y, y^2, y c.
//
// One lane per pair, a pure gather: 4 (2) bytes of X and 4 of Ct per pair and frame, plus 4 per other, against 3 fp64
// operations and 2 widenings.  The host sorts the pairs by (ROI, pixel), so adjacent lanes read adjacent pixels of a window
// row (segments of a window's width) and pair_k is the same in almost every lane of a wave, whose trace load is then one
// address; the Ct block (K x 1024 floats) stays in L2.  The loads of RW_U frames are issued before their use.  The others
// run in the outer loop and the RW_U frames in the inner one, so the tables are read once per RW_U frames; per frame the
// subtractions still come in stored order, and frames do not interact.
//
// Order of the arithmetic: contraction is off, every fp32 operation is rounded on its own; both products are (double) a *
// (double) b of two fp32 values, exact, so the fused multiply-add rounds as the product followed by the sum does; every sum
// is one fp64 chain per pair over the frames in ascending order, started from the value stored in mom and stored back
// once.  The bits of pair i depend on its pixel's column, the trace rows it names, its oth_a and the stored state only: not
// on how the frames are split over calls, on ldx or ldct, on the element type holding the same values, on the pair's
// position in the table or on what other pairs are present.  One owner per pair: no atomics, no LDS, no workspace, no
// synchronisation.
#include "pmd_common.h"
#include "../../include/pmd_hip.h"

namespace {

constexpr int RW_THREADS = 256;
constexpr int RW_U = 8;               // frames whose loads are in flight per lane

template <typename E>
__global__ __launch_bounds__(RW_THREADS) void roi_window_moments_kernel(const E* __restrict__ X, long ldx, int n,
                                                                        const float* __restrict__ Ct, long ldct, long n_pairs,
                                                                        const int* __restrict__ pair_px,
                                                                        const int* __restrict__ pair_k,
                                                                        const int64_t* __restrict__ oth_ptr,
                                                                        const int* __restrict__ oth_k,
                                                                        const float* __restrict__ oth_a,
                                                                        double* __restrict__ mom) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * RW_THREADS + threadIdx.x;
  if (i >= n_pairs) return;
  const long px = pair_px[i];
  const long k = pair_k[i];
  const long q0 = oth_ptr[i], q1 = oth_ptr[i + 1];
  double s_y = mom[i], s_yy = mom[n_pairs + i], s_yc = mom[2 * n_pairs + i];

  for (int fs = 0; fs < n; fs += RW_U) {
    float y[RW_U], c[RW_U];
    long fx[RW_U], fc[RW_U];
#pragma unroll
    for (int u = 0; u < RW_U; ++u) {
      const long f = min(fs + u, n - 1);                     // past the end: re-read the last frame, not used
      fx[u] = f * ldx;
      fc[u] = f * ldct;
      y[u] = (float)X[fx[u] + px];
      c[u] = Ct[fc[u] + k];
    }
    for (long q = q0; q < q1; ++q) {
      const float a = oth_a[q];
      const long ko = oth_k[q];
#pragma unroll
      for (int u = 0; u < RW_U; ++u) y[u] = y[u] - a * Ct[fc[u] + ko];
    }
#pragma unroll
    for (int u = 0; u < RW_U; ++u) {
      if (fs + u < n) {                                      // the same in every lane
        const double a = (double)y[u];
        s_y = s_y + a;
        s_yy = __builtin_fma(a, a, s_yy);
        s_yc = __builtin_fma(a, (double)c[u], s_yc);
      }
    }
  }
  mom[i] = s_y;
  mom[n_pairs + i] = s_yy;
  mom[2 * n_pairs + i] = s_yc;
}

}  // namespace

extern "C" {

int pmd_roi_window_moments_accumulate(pmd_ctx* ctx, const void* X, int elem, long ldx, long D, int n, const float* Ct,
                                      long ldct, int K, long n_pairs, const int* pair_px, const int* pair_k,
                                      const int64_t* oth_ptr, const int* oth_k, const float* oth_a, double* mom) {
  CTX_CHECK(ctx);
  const char* what = "pmd_roi_window_moments_accumulate";
  if (n < 1 || K < 1 || D < 1) return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (n >= 1, K >= 1, D >= 1)");
  if (ldx < D) return pmd_fail(ctx, PMD_ERR_ARG, what, "ldx < D");
  if (ldct < K) return pmd_fail(ctx, PMD_ERR_ARG, what, "ldct < K");
  if (n_pairs < 0) return pmd_fail(ctx, PMD_ERR_ARG, what, "n_pairs < 0");
  if (pmd_bad_elem(elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown element type");
  if (n_pairs == 0) return PMD_OK;
  if (!X || !Ct || !pair_px || !pair_k || !oth_ptr || !oth_k || !oth_a || !mom)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  const long blocks = (n_pairs + RW_THREADS - 1) / RW_THREADS;
  if (blocks > 0x7fffffffL) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many pairs in one call");
  pmd_prof_scope prof__(ctx, "roi_window_moments_accumulate");
  pmd_with_elem(elem, [&](auto e) {
    using E = typename decltype(e)::type;
    hipLaunchKernelGGL((roi_window_moments_kernel<E>), dim3((unsigned)blocks), dim3(RW_THREADS), 0, ctx->stream, (const E*)X,
                       ldx, n, Ct, ldct, n_pairs, pair_px, pair_k, oth_ptr, oth_k, oth_a, mom);
  });
  PMD_LAUNCH_CHECK(ctx, "roi_window_moments_kernel");
  return PMD_OK;
}

}  // extern "C"
