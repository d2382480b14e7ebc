// Per-pixel regressor maps (localmd_amd/maps.py):  acc[k][c] += sum_f X[k][f] * z[f][c],  z[f][c] = (float) Y[f][c] - mean[c],
// for one block of n <= 1024 frames of a frames-first batch Y (float32 / uint16 / int16, converted and centred in
// registers) against K time courses X, with the moments sum_f z and sum_f z^2 of every pixel on the side.  It is the
// tall-skinny product X Z: the batch is the big operand and is read once, in its own element type.
//
// One wave owns a strip of 128 consecutive pixels and walks all n frames of it; a workgroup is four neighbouring strips.
// Lane l reads RG_PX = 4 consecutive pixels c0 + 4 (l & 31) .. + 3 of frame f + (l >> 5) in one load (8 bytes of uint16,
// 16 of float32; a misaligned batch or a strip that crosses D reads them one by one on clamped indices) and feeds them
// as the B operands of four v_mfma_f32_32x32x2_f32 (B[k = l >> 5][j = l & 31]): MFMA t of the lane's four computes the
// pixels c0 + 4 j + t.  The A operand is the regressor tile A[i = l & 31][k = l >> 5] = X[32 g + i][f + k], read from
// LDS, where the workgroup stages the regressors of RG_FC = 64 frames at a time ([frame][k], row stride 32 G + 1: the
// staging writes of 64 consecutive frames hit 64 banks).  A launch keeps the accumulator tiles of G <= 4 groups of 32
// regressors in registers (64 G per lane), so the batch is read once for K <= 128; larger K go in launches of 128 rows.
// K is padded to 32 G with zero rows, an odd n with a zero column of X and a zero z (the padded frame's load re-reads
// frame n - 1 and never leaves the batch).  A step is U frame pairs whose loads are all issued before its first MFMA, and
// a step is always whole: a short block (the last of a movie) still loads and multiplies up to U - 1 pairs of zeros, at
// n = 1 and G = 1 sixteen loads of the clamped frame and 64 MFMAs; a cost on one block per movie, not on the bits.
//
// Arithmetic: the MFMA is bit for bit the fmaf chain  s = fmaf(X[k][f], z[f][c], s)  over f = 0, 1, ..., n - 1 from 0.f,
// each output element on its own; it is converted to double and added to acc once.  The moments are two chains per lane
// and pixel over the frames of the lane's parity, f = h, h + 2, ... (s1 += z, s2 = fmaf(z, z, s2)), the two parities are
// added and the sum goes to mom once.  Every element has one owner: no atomics, and the order depends on n alone.
#include "pmd_common.h"
#include "../../include/pmd_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int RG_PX = 4;              // consecutive pixels per lane
constexpr int RG_STRIP = 32 * RG_PX;  // pixels per wave
constexpr int RG_WG = 4 * RG_STRIP;   // pixels per workgroup
constexpr int RG_FC = 64;             // frames of X staged per round
constexpr int RG_GMAX = 4;            // groups of 32 regressors per launch at most

template <typename E>
struct alignas(RG_PX * sizeof(E)) rg_vec {
  E e[RG_PX];
};

// U: frame pairs in flight per lane (their loads are issued before the first MFMA of the step)
template <typename E, int G, int U>
__global__ __launch_bounds__(256) void regress_kernel(const E* __restrict__ Y, long ldy, int n, long D,
                                                      const float* __restrict__ mean, const float* __restrict__ X,
                                                      long ldx, int K, double* __restrict__ acc, long lda,
                                                      double* __restrict__ mom, int vec_ok) {
  constexpr int KS = 32 * G + 1;      // LDS row stride
  __shared__ float Xs[RG_FC * KS];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lj = lane & 31, lh = lane >> 5;
  const long c = (long)blockIdx.x * RG_WG + (long)w * RG_STRIP + RG_PX * lj;   // first pixel of this lane
  const bool full = vec_ok && c + RG_PX <= D;
  long cj[RG_PX];                      // clamped pixel ids (lanes beyond D re-read pixel D - 1; never stored)
  float mu[RG_PX];
#pragma unroll
  for (int t = 0; t < RG_PX; ++t) {
    cj[t] = c + t < D ? c + t : D - 1;
    mu[t] = mean ? mean[cj[t]] : 0.f;
  }
  f32x16 a[G][RG_PX];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int t = 0; t < RG_PX; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) a[g][t][v] = 0.f;
  float s1[RG_PX], s2[RG_PX];
#pragma unroll
  for (int t = 0; t < RG_PX; ++t) s1[t] = s2[t] = 0.f;

  for (int f0 = 0; f0 < n; f0 += RG_FC) {
    // stage X[:, f0 .. f0 + 63] as Xs[frame][k]; zeros beyond K and n
    __syncthreads();
    for (int i = tid; i < RG_FC * 32 * G; i += 256) {
      const int fl = i & (RG_FC - 1), k = i / RG_FC;
      const bool ok = k < K && f0 + fl < n;
      Xs[fl * KS + k] = ok ? X[(long)k * ldx + f0 + fl] : 0.f;
    }
    __syncthreads();
    const int nfc = min(RG_FC, n - f0);
    for (int p0 = 0; 2 * p0 < nfc; p0 += U) {
      float y[U][RG_PX];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int f = f0 + 2 * (p0 + u) + lh;
        const E* row = Y + (long)min(f, n - 1) * ldy;
        if (full) {
          const rg_vec<E> v = *reinterpret_cast<const rg_vec<E>*>(row + c);
#pragma unroll
          for (int t = 0; t < RG_PX; ++t) y[u][t] = (float)v.e[t];
        } else {
#pragma unroll
          for (int t = 0; t < RG_PX; ++t) y[u][t] = (float)row[cj[t]];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int fl = 2 * (p0 + u) + lh;            // < RG_FC: U divides RG_FC / 2; rows from n on hold zeros
        const bool fv = f0 + fl < n;
        float z[RG_PX];
#pragma unroll
        for (int t = 0; t < RG_PX; ++t) {
          z[t] = fv ? y[u][t] - mu[t] : 0.f;
          s1[t] += z[t];
          s2[t] = __builtin_fmaf(z[t], z[t], s2[t]);
        }
        const float* xr = Xs + fl * KS + lj;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float xa = xr[32 * g];
#pragma unroll
          for (int t = 0; t < RG_PX; ++t) a[g][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa, z[t], a[g][t], 0, 0, 0);
        }
      }
    }
  }

  // D map of 32x32x2: column (pixel 4 j + t) j = lane & 31, rows (regressors) (v & 3) + 8 (v >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int k = 32 * g + (v & 3) + 8 * (v >> 2) + 4 * lh;
      if (k < K) {
        double* o = acc + (long)k * lda + c;
#pragma unroll
        for (int t = 0; t < RG_PX; ++t)
          if (c + t < D) o[t] += (double)a[g][t][v];
      }
    }
  if (mom) {
#pragma unroll
    for (int t = 0; t < RG_PX; ++t) {
      const float m1 = s1[t] + __shfl_xor(s1[t], 32, 64);
      const float m2 = s2[t] + __shfl_xor(s2[t], 32, 64);
      if (lh == 0 && c + t < D) {
        mom[c + t] += (double)m1;
        mom[D + c + t] += (double)m2;
      }
    }
  }
}

template <typename E, int G>
void launch_g(pmd_ctx* ctx, dim3 grid, const void* Y, long ldy, int n, long D, const float* mean, const float* X, long ldx,
              int K, double* acc, long lda, double* mom) {
  const int vec_ok = ldy % RG_PX == 0 && ((uintptr_t)Y % (RG_PX * sizeof(E))) == 0;
  constexpr int U = G == 1 ? 16 : 8;
  hipLaunchKernelGGL((regress_kernel<E, G, U>), grid, dim3(256), 0, ctx->stream, (const E*)Y, ldy, n, D, mean, X, ldx, K,
                     acc, lda, mom, vec_ok);
}

template <typename E>
void launch_e(pmd_ctx* ctx, dim3 grid, const void* Y, long ldy, int n, long D, const float* mean, const float* X, long ldx,
              int K, double* acc, long lda, double* mom) {
  switch ((K + 31) / 32) {
    case 0:
    case 1: launch_g<E, 1>(ctx, grid, Y, ldy, n, D, mean, X, ldx, K, acc, lda, mom); break;
    case 2: launch_g<E, 2>(ctx, grid, Y, ldy, n, D, mean, X, ldx, K, acc, lda, mom); break;
    case 3: launch_g<E, 3>(ctx, grid, Y, ldy, n, D, mean, X, ldx, K, acc, lda, mom); break;
    default: launch_g<E, 4>(ctx, grid, Y, ldy, n, D, mean, X, ldx, K, acc, lda, mom); break;
  }
}

}  // namespace

extern "C" {

int pmd_regress_accumulate(pmd_ctx* ctx, const void* Y, int elem, long ldy, int n, long D, const float* mean,
                           const float* X, long ldx, int K, double* acc, long lda, double* mom) {
  CTX_CHECK(ctx);
  const char* what = "pmd_regress_accumulate";
  if (n < 0 || D < 1 || K < 0 || ldy < D || (K > 0 && (ldx < n || lda < D)))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (n, K >= 0, D >= 1, ldy, lda >= D, ldx >= n)");
  if (n > PMD_REGRESS_BLOCK) return pmd_fail(ctx, PMD_ERR_ARG, what, "n > PMD_REGRESS_BLOCK frames in one call");
  if (pmd_bad_elem(elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown element type");
  if (n == 0 || (K == 0 && !mom)) return PMD_OK;
  if (!Y || (K > 0 && (!X || !acc))) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  const long n_wg = (D + RG_WG - 1) / RG_WG;
  if (n_wg > 0x7fffffffL) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many pixels in one call");
  pmd_prof_scope prof__(ctx, "regress_accumulate");
  const dim3 grid((unsigned)n_wg);
  constexpr int KL = 32 * RG_GMAX;    // regressors per launch; the moments are formed by the first one
  int k0 = 0;
  do {
    const int kn = K - k0 < KL ? K - k0 : KL;
    const float* x = X ? X + (long)k0 * ldx : nullptr;
    double* a = acc ? acc + (long)k0 * lda : nullptr;
    double* m = k0 == 0 ? mom : nullptr;
    pmd_with_elem(elem, [&](auto e) {
      launch_e<typename decltype(e)::type>(ctx, grid, Y, ldy, n, D, mean, x, ldx, kn, a, lda, m);
    });
    k0 += KL;
  } while (k0 < K);
  PMD_LAUNCH_CHECK(ctx, "regress_kernel");
  return PMD_OK;
}

}  // extern "C"
