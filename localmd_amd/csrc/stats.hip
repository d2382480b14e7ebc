// Per-pixel summary images (localmd_amd/summary.py): the running minimum and maximum of every pixel (optionally of the
// means of `bin` consecutive frames) with the frame that first attains them, and the sums of z, z^2, z^3, z^4 of
// z[f][c] = (float) Y[f][c] - centre[c], for one block of n <= 1024 frames of a frames-first batch Y (float32 / uint16 /
// int16, converted in registers).  Purely memory-bound: the block is read once, in its own element type.
//
// A workgroup is four waves and owns 64 V consecutive pixels, V = 4 (float32) or 8 (16-bit): lane l of every wave reads
// the V pixels c = (64 blockIdx + l) V .. + V - 1 of a frame in one 16-byte load (a row that is not 16-byte aligned, or a
// lane whose run crosses D, reads them one by one on clamped indices; the arithmetic below is the same, so are the
// bits).  Wave w walks the frames of slice w, [256 w, min(n, 256 w + 256)), in ascending order, ST_U frames' loads issued
// ahead of their use; a slice from n on is empty.  The slices do not depend on bin, D, ldy or the element type.
//
// Order of the arithmetic (fixed by n for the moments, by (n, bin) for the extrema):
//   moments  per slice one fp32 chain per sum over its frames in ascending order from 0.f (s1 += z, s2 += z2, s3 += z2 z,
//            s4 += z2 z2 with z2 = z z; every product and sum rounded on its own, no fma); the slice sums are added in
//            ascending slice order, ((p0 + p1) + p2) + p3 over the slices that hold frames; the result is converted to
//            double and added to mom once.
//   bin == 1 the value of frame f is (float) Y[f][c] itself.
//   bin > 1  bins start at multiples of bin (f0 is one).  bin <= 256: a bin lies in one slice; its value is the fp32 chain
//            over its frames in ascending order starting from the first frame's value, divided (IEEE) by its frame count
//            (the block's last bin may be short).  bin = 512, 1024: the chain of every slice of the bin is formed in the
//            same way, the slice sums are added in ascending slice order starting from the first, then divided.
//   extrema  a value replaces the running minimum only on <, the maximum only on >, values taken in ascending frame
//            order within a slice, slices combined in ascending order, and the block against the state last: the first
//            frame that attains an extremum keeps arg, within a call and across calls; NaN never compares true.
// The partial results of waves 1..3 reach wave 0 through LDS, one slice per round; wave 0 owns every pixel's state: no
// atomics.  Launches nothing but the kernel: no synchronisation, no allocation, no workspace.
#include "pmd_common.h"
#include "../../include/pmd_hip.h"

namespace {

constexpr int ST_SLICE = 256;         // frames per wave
constexpr int ST_WAVES = PMD_STATS_BLOCK / ST_SLICE;
constexpr int ST_U = 8;               // frames whose loads are in flight per lane

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <typename E>
union st_vec {                        // 16 bytes of a frame: one load, or V elements one by one
  u32x4 q;
  E e[16 / sizeof(E)];
};

template <typename E, bool EXT, bool MOM>
__global__ __launch_bounds__(64 * ST_WAVES) void stats_kernel(const E* __restrict__ Y, long ldy, int n, long D, int f0,
                                                               int bin, const float* __restrict__ centre,
                                                               float* __restrict__ ext, int* __restrict__ arg,
                                                               double* __restrict__ mom, int vec_ok) {
#pragma clang fp contract(off)
  constexpr int V = 16 / sizeof(E);
  constexpr int ITEMS = V * ((EXT ? 4 : 0) + (MOM ? 4 : 0));
  __shared__ float part[ITEMS * 64];   // [item][lane]: the partial results of one slice
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long c = ((long)blockIdx.x * 64 + lane) * V;   // first pixel of this lane
  const bool full = vec_ok && c + V <= D;
  long cj[V];                          // clamped pixel ids (lanes beyond D re-read pixel D - 1; never stored)
  float mu[V];
#pragma unroll
  for (int t = 0; t < V; ++t) {
    cj[t] = c + t < D ? c + t : D - 1;
    mu[t] = MOM && centre ? centre[cj[t]] : 0.f;
  }
  const float inf = __builtin_inff();
  float lo[V], hi[V], bs[V], s1[V], s2[V], s3[V], s4[V];
  int alo[V], ahi[V];
#pragma unroll
  for (int t = 0; t < V; ++t) {
    lo[t] = inf, hi[t] = -inf, alo[t] = ahi[t] = -1;
    bs[t] = s1[t] = s2[t] = s3[t] = s4[t] = 0.f;
  }
  const bool big = bin > ST_SLICE;     // a bin spans whole slices: the walk leaves the slice's chain in bs
  const int fmask = (big ? ST_SLICE : bin) - 1;
  const int fa = w * ST_SLICE, fb = min(n, fa + ST_SLICE);

  for (int fs = fa; fs < fb; fs += ST_U) {
    st_vec<E> y[ST_U];
#pragma unroll
    for (int u = 0; u < ST_U; ++u) {
      const E* row = Y + (long)min(fs + u, fb - 1) * ldy;   // past the slice: re-read its last frame, not used
      if (full) {
        y[u].q = *reinterpret_cast<const u32x4*>(row + c);
      } else {
#pragma unroll
        for (int t = 0; t < V; ++t) y[u].e[t] = row[cj[t]];
      }
    }
#pragma unroll
    for (int u = 0; u < ST_U; ++u) {
      const int f = fs + u;
      if (f < fb) {                    // the same in every lane
        if (MOM) {
#pragma unroll
          for (int t = 0; t < V; ++t) {
            const float z = (float)y[u].e[t] - mu[t];
            const float z2 = z * z;
            s1[t] = s1[t] + z;
            s2[t] = s2[t] + z2;
            s3[t] = s3[t] + z2 * z;
            s4[t] = s4[t] + z2 * z2;
          }
        }
        if (EXT) {
          if (bin == 1) {
#pragma unroll
            for (int t = 0; t < V; ++t) {
              const float v = (float)y[u].e[t];
              if (v < lo[t]) lo[t] = v, alo[t] = f0 + f;
              if (v > hi[t]) hi[t] = v, ahi[t] = f0 + f;
            }
          } else {
            const int k = f & fmask;   // position of the frame in its bin (in its slice for a big bin)
#pragma unroll
            for (int t = 0; t < V; ++t) bs[t] = k == 0 ? (float)y[u].e[t] : bs[t] + (float)y[u].e[t];
            if (!big && (k == fmask || f == n - 1)) {
              const float cnt = (float)(k + 1);
#pragma unroll
              for (int t = 0; t < V; ++t) {
                const float v = bs[t] / cnt;
                if (v < lo[t]) lo[t] = v, alo[t] = f0 + f - k;
                if (v > hi[t]) hi[t] = v, ahi[t] = f0 + f - k;
              }
            }
          }
        }
      }
    }
  }

  // wave 0, big bins only: the bin of slice s is complete with s when s is its last slice or the block's last
  auto close_bin = [&](int s) {
    const int per = bin / ST_SLICE;
    if ((s + 1) % per != 0 && (s + 1) * ST_SLICE < n) return;
    const int b0 = s / per * bin;
    const float cnt = (float)(min(n, b0 + bin) - b0);
#pragma unroll
    for (int t = 0; t < V; ++t) {
      const float v = bs[t] / cnt;
      if (v < lo[t]) lo[t] = v, alo[t] = f0 + b0;
      if (v > hi[t]) hi[t] = v, ahi[t] = f0 + b0;
    }
  };
  if (EXT && big && w == 0) close_bin(0);

  for (int s = 1; s < ST_WAVES && s * ST_SLICE < n; ++s) {   // the same trip count in every wave of the grid
    __syncthreads();
    if (w == s) {
      int i = 0;
#pragma unroll
      for (int t = 0; t < V; ++t) {
        if (EXT) {
          part[(i++) * 64 + lane] = big ? bs[t] : lo[t];
          part[(i++) * 64 + lane] = hi[t];
          part[(i++) * 64 + lane] = __int_as_float(alo[t]);
          part[(i++) * 64 + lane] = __int_as_float(ahi[t]);
        }
        if (MOM) {
          part[(i++) * 64 + lane] = s1[t];
          part[(i++) * 64 + lane] = s2[t];
          part[(i++) * 64 + lane] = s3[t];
          part[(i++) * 64 + lane] = s4[t];
        }
      }
    }
    __syncthreads();
    if (w == 0) {
      int i = 0;
#pragma unroll
      for (int t = 0; t < V; ++t) {
        if (EXT) {
          const float plo = part[(i++) * 64 + lane], phi = part[(i++) * 64 + lane];
          const int palo = __float_as_int(part[(i++) * 64 + lane]), pahi = __float_as_int(part[(i++) * 64 + lane]);
          if (big) {
            bs[t] = s % (bin / ST_SLICE) == 0 ? plo : bs[t] + plo;
          } else {
            if (plo < lo[t]) lo[t] = plo, alo[t] = palo;
            if (phi > hi[t]) hi[t] = phi, ahi[t] = pahi;
          }
        }
        if (MOM) {
          s1[t] = s1[t] + part[(i++) * 64 + lane];
          s2[t] = s2[t] + part[(i++) * 64 + lane];
          s3[t] = s3[t] + part[(i++) * 64 + lane];
          s4[t] = s4[t] + part[(i++) * 64 + lane];
        }
      }
      if (EXT && big) close_bin(s);
    }
  }

  if (w != 0) return;
#pragma unroll
  for (int t = 0; t < V; ++t) {
    if (c + t >= D) continue;
    const long p = c + t;
    if (EXT) {
      if (lo[t] < ext[p]) {
        ext[p] = lo[t];
        if (arg) arg[p] = alo[t];
      }
      if (hi[t] > ext[D + p]) {
        ext[D + p] = hi[t];
        if (arg) arg[D + p] = ahi[t];
      }
    }
    if (MOM) {
      mom[p] += (double)s1[t];
      mom[D + p] += (double)s2[t];
      mom[2 * D + p] += (double)s3[t];
      mom[3 * D + p] += (double)s4[t];
    }
  }
}

template <typename E>
void launch_e(pmd_ctx* ctx, const void* Y, long ldy, int n, long D, int f0, int bin, const float* centre, float* ext,
              int* arg, double* mom) {
  constexpr int V = 16 / sizeof(E);
  const dim3 grid((unsigned)((D + 64 * V - 1) / (64 * V))), block(64 * ST_WAVES);
  const int vec_ok = (ldy * sizeof(E)) % 16 == 0 && (uintptr_t)Y % 16 == 0;
  const E* y = (const E*)Y;
  if (ext && mom)
    hipLaunchKernelGGL((stats_kernel<E, true, true>), grid, block, 0, ctx->stream, y, ldy, n, D, f0, bin, centre, ext, arg,
                       mom, vec_ok);
  else if (ext)
    hipLaunchKernelGGL((stats_kernel<E, true, false>), grid, block, 0, ctx->stream, y, ldy, n, D, f0, bin, centre, ext,
                       arg, mom, vec_ok);
  else
    hipLaunchKernelGGL((stats_kernel<E, false, true>), grid, block, 0, ctx->stream, y, ldy, n, D, f0, bin, centre, ext,
                       arg, mom, vec_ok);
}

}  // namespace

extern "C" {

int pmd_pixel_stats_accumulate(pmd_ctx* ctx, const void* Y, int elem, long ldy, int n, long D, long f0, int bin,
                               const float* centre, float* ext, int* arg, double* mom) {
  CTX_CHECK(ctx);
  const char* what = "pmd_pixel_stats_accumulate";
  if (n < 1 || n > PMD_STATS_BLOCK) return pmd_fail(ctx, PMD_ERR_ARG, what, "n outside 1 .. PMD_STATS_BLOCK");
  if (D < 1 || ldy < D) return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (D >= 1, ldy >= D)");
  if (bin < 1 || bin > PMD_STATS_BLOCK || (bin & (bin - 1)) != 0)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "bin is not a power of two in 1 .. PMD_STATS_BLOCK");
  if (f0 < 0 || f0 % bin != 0 || f0 + n >= 0x80000000L)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "f0 is negative, not a multiple of bin, or f0 + n >= 2^31");
  if (pmd_bad_elem(elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown element type");
  if (!ext && !mom) return pmd_fail(ctx, PMD_ERR_ARG, what, "ext and mom are both NULL");
  if (arg && !ext) return pmd_fail(ctx, PMD_ERR_ARG, what, "arg without ext");
  if (!Y) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if ((D + 255) / 256 > 0x7fffffffL) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many pixels in one call");
  pmd_prof_scope prof__(ctx, "pixel_stats_accumulate");
  pmd_with_elem(elem, [&](auto e) {
    launch_e<typename decltype(e)::type>(ctx, Y, ldy, n, D, (int)f0, bin, centre, ext, arg, mom);
  });
  PMD_LAUNCH_CHECK(ctx, "stats_kernel");
  return PMD_OK;
}

}  // extern "C"
