// Non-negative Gauss-Seidel (HALS) sweeps of the demixing solver (localmd_amd/demix.py): x ~ A c + b with footprints
// A >= 0 on fixed supports and traces C.  Two kernels, one launch per sweep each; contraction is off and every operation
// is rounded on its own in a fixed order, so tests/hals_ref.py reproduces the sweep over frames bit for bit.
//
// hals_sweep_kernel   over frames, with the sparse G = A^T A.  A lane owns one column t of C and runs the whole k loop on
//                     it: columns are independent, so no workgroup waits for another, and the rows of C and P are read
//                     and written coalesced along t.  Row k of G (indptr, indices, data, invd, lo) is the same in every
//                     lane: the loads are wave-uniform and go through the scalar cache, once per wave and k, not once per
//                     lane.  A lane reads the C[j][t] it wrote itself for j < k (program order), nobody else's.
// hals_pixels_kernel  over pixels, with the dense H = C~ C~^T.  One wave per pixel q.  For each ROI j covering q the
//                     lanes stride the nonzeros of the pixel's U row (lane l: l, l + 64, ... in one chain from 0), an xor
//                     butterfly (1, 2, ..., 32) folds the lanes, and lane j keeps Sy_j = scale[q] * sum.  Lane j also
//                     holds a_j and k_j; the Gauss-Seidel step for j forms a_j' H[k_j'][k_j] in lane j' (the gathered
//                     column of H), folds it with the same butterfly, and lane j takes the new value, which the next
//                     step reads.  No LDS: the per-pixel state is one register per lane, and at most 64 ROIs cover a
//                     pixel.  A wave only ever writes the pairs of its own pixel.
#include "pmd_common.h"
#include "../../include/pmd_hip.h"

namespace {

constexpr int HALS_THREADS = 256;
constexpr int HALS_WAVES = HALS_THREADS / 64;

__global__ __launch_bounds__(HALS_THREADS) void hals_sweep_kernel(float* C, long ldc, const float* __restrict__ P, long ldp,
                                                                   int K, long n, const int64_t* __restrict__ indptr,
                                                                   const int* __restrict__ indices,
                                                                   const float* __restrict__ data,
                                                                   const float* __restrict__ invd,
                                                                   const float* __restrict__ lo) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * HALS_THREADS + threadIdx.x;
  if (t >= n) return;
  for (int k = 0; k < K; ++k) {
    const float iv = invd[k];
    if (iv == 0.f) continue;           // the same in every lane
    const long i0 = indptr[k], i1 = indptr[k + 1];
    float acc = P[(long)k * ldp + t];
    for (long i = i0; i < i1; ++i) {
      const float g = data[i];
      const float c = C[(long)indices[i] * ldc + t];
      const float prod = g * c;
      acc = acc - prod;
    }
    const float step = acc * iv;
    const float v = C[(long)k * ldc + t] + step;
    const float l = lo[k];
    C[(long)k * ldc + t] = v < l ? l : v;
  }
}

__device__ __forceinline__ float hals_wave_sum(float v) {
#pragma clang fp contract(off)
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
  return v;
}

__global__ __launch_bounds__(HALS_THREADS) void hals_pixels_kernel(long n_px, const int* __restrict__ px_row,
                                                                    const int64_t* __restrict__ cov_ptr,
                                                                    const int* __restrict__ cov_k, float* a,
                                                                    const int64_t* __restrict__ u_indptr,
                                                                    const int* __restrict__ u_indices,
                                                                    const float* __restrict__ u_data,
                                                                    const float* __restrict__ scale,
                                                                    const float* __restrict__ Mt, long ldm,
                                                                    const float* __restrict__ H, long ldh,
                                                                    const int* __restrict__ frozen) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const long q = (long)blockIdx.x * HALS_WAVES + (threadIdx.x >> 6);     // the same in every lane of a wave
  if (q >= n_px) return;
  const long c0 = cov_ptr[q];
  const int nc = (int)(cov_ptr[q + 1] - c0);
  if (nc < 1 || nc > PMD_HALS_MAX_COVER) return;                          // the host refuses such tables
  const long row = px_row[q];
  const long i0 = u_indptr[row], i1 = u_indptr[row + 1];
  const float sc = scale[q];
  const bool mine = lane < nc;
  const int kj = mine ? cov_k[c0 + lane] : 0;
  float aj = mine ? a[c0 + lane] : 0.f;
  const float hjj = mine ? H[(long)kj * ldh + kj] : 0.f;
  const bool skip = !mine || hjj == 0.f || frozen[kj] != 0;

  float sy = 0.f;
  for (int j = 0; j < nc; ++j) {
    const long kk = __shfl(kj, j, 64);
    const float* m = Mt + kk * ldm;
    float s = 0.f;
    for (long i = i0 + lane; i < i1; i += 64) {
      const float prod = u_data[i] * m[u_indices[i]];
      s = s + prod;
    }
    s = hals_wave_sum(s);
    if (lane == j) sy = sc * s;
  }
  for (int j = 0; j < nc; ++j) {
    const long kk = __shfl(kj, j, 64);
    const float term = mine ? aj * H[(long)kj * ldh + kk] : 0.f;
    const float dot = hals_wave_sum(term);
    if (lane == j && !skip) {
      const float r = sy - dot;
      const float v = aj + r / hjj;
      aj = v < 0.f ? 0.f : v;
    }
  }
  if (!skip) a[c0 + lane] = aj;
}

}  // namespace

extern "C" {

int pmd_hals_sweep(pmd_ctx* ctx, float* C, long ldc, const float* P, long ldp, int K, long n, const int64_t* indptr,
                   const int* indices, const float* data, const float* invd, const float* lo) {
  CTX_CHECK(ctx);
  const char* what = "pmd_hals_sweep";
  if (K < 1 || n < 0 || ldc < n || ldp < n)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (K >= 1, n >= 0, ldc >= n, ldp >= n)");
  if (!C || !P || !indptr || !indices || !data || !invd || !lo) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if (n == 0) return PMD_OK;
  const long blocks = (n + HALS_THREADS - 1) / HALS_THREADS;
  if (blocks > 0x7fffffffL) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many columns in one call");
  pmd_prof_scope prof__(ctx, "hals_sweep");
  hipLaunchKernelGGL(hals_sweep_kernel, dim3((unsigned)blocks), dim3(HALS_THREADS), 0, ctx->stream, C, ldc, P, ldp, K, n,
                     indptr, indices, data, invd, lo);
  PMD_LAUNCH_CHECK(ctx, "hals_sweep_kernel");
  return PMD_OK;
}

int pmd_hals_pixels(pmd_ctx* ctx, long n_px, const int* px_row, const int64_t* cov_ptr, const int* cov_k, float* a,
                    const int64_t* u_indptr, const int* u_indices, const float* u_data, const float* scale,
                    const float* Mt, long ldm, const float* H, long ldh, const int* frozen) {
  CTX_CHECK(ctx);
  const char* what = "pmd_hals_pixels";
  if (n_px < 0 || ldm < 0 || ldh < 1) return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (n_px, ldm >= 0, ldh >= 1)");
  if (!px_row || !cov_ptr || !cov_k || !a || !u_indptr || !u_indices || !u_data || !scale || !Mt || !H || !frozen)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if (n_px == 0) return PMD_OK;
  const long blocks = (n_px + HALS_WAVES - 1) / HALS_WAVES;
  if (blocks > 0x7fffffffL) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many pixels in one call");
  pmd_prof_scope prof__(ctx, "hals_pixels");
  hipLaunchKernelGGL(hals_pixels_kernel, dim3((unsigned)blocks), dim3(HALS_THREADS), 0, ctx->stream, n_px, px_row, cov_ptr,
                     cov_k, a, u_indptr, u_indices, u_data, scale, Mt, ldm, H, ldh, frozen);
  PMD_LAUNCH_CHECK(ctx, "hals_pixels_kernel");
  return PMD_OK;
}

}  // extern "C"
