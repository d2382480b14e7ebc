// Rolling-baseline dF/F (localmd_amd/baseline.py): the time series of every pixel is reduced to knots (the means of bins
// of `bin` frames, pmd_bin_means), the knots go through a sliding minimum and / or maximum along time
// (pmd_sliding_extremum) or a sliding order statistic (pmd_sliding_quantile), and every frame is compared with the baseline interpolated between the knots
// (pmd_baseline_apply).  All three stream frames-first matrices: lane l of a wave owns V consecutive pixels, V = 4 (fp32)
// or 8 (16-bit), one 16-byte load per frame (a row that is not 16-byte aligned, or a lane whose run crosses N, moves them
// one by one on clamped indices; the arithmetic is the same, so are the bits), and walks time inside the thread, BL_U
// frames' loads issued ahead of their use.  The waves of a workgroup take different time slices of the same pixels; no
// wave needs another's result, so there is no LDS and no barrier.  Contraction is off: every operation is rounded on
// its own.
//
// bin_means_kernel    a wave takes a slice of max(bin, 64) frames (whole bins).  The value of a bin is the fp32 chain over
//                     its frames in ascending order starting from the first frame's value, divided (IEEE) by its frame
//                     count; bin == 1 stores (float) y itself.
// extremum_kernel     van Herk / Gil-Werman with W = 2 half + 1: a wave takes the W outputs j = s W .. s W + W - 1 of
//                     segment s.  The window [j - half, j + half] is cut at m = s W + half: a backward scan from m down
//                     leaves B[j] = ext(x[j - half .. m]) in the workspace row j, a forward scan from m up keeps
//                     F = ext(x[m .. j + half]) in registers, out[j] = ext(B[j], F).  Two loads of x, one store and one
//                     load of B and one store of out per output, whatever half is.  Frames outside [0, n) are virtual
//                     padding that never wins: the scans start from NaN, which fminf / fmaxf drop against any value (as
//                     they drop +inf / -inf padding against any value but NaN), so a window is NaN only when every frame
//                     it really holds is.
// quantile_kernel     the sliding order statistic, on the integer keys of quantile.hip.  A wave takes a slice of BL_QSLICE
//                     consecutive outputs.  The first is selected by bisection on the 32 key bits, one counting scan
//                     of the window per bit.  From then on each column keeps its answer key a with cl = #{key < a} and
//                     ce = #{key == a}; the next window loses one member and gains one, two compares each update cl
//                     and ce, and the answer stays while cl <= rank < cl + ce.  Otherwise it moves to the neighbouring
//                     distinct key, which one scan of the window finds together with its count.  The scan runs when
//                     any lane of the wave needs it, which with 256 columns per wave is nearly every step: the work
//                     is one scan per output plus 33 per slice.  A scan reads the rows the window really holds once
//                     and counts the replicated first and last row with a multiplicity, so it is min(W, n) rows
//                     whatever half is.  Integer work only: no workspace, and nothing to round.
// apply_kernel        a wave takes a slice of 32 frames.  Per frame the bin j whose centre is the last at or before the
//                     frame and the weight w are the same in every lane; the knot rows j and j + 1 stay in registers
//                     until j moves on.
#include "pmd_common.h"
#include "../../include/pmd_hip.h"

namespace {

constexpr int BL_WAVES = 4;
constexpr int BL_U = 8;               // frames whose loads are in flight per lane
constexpr int BL_APPLY_SLICE = 32;    // frames per wave of apply_kernel
constexpr int BL_MIN_SLICE = 64;      // frames per wave of bin_means_kernel, at least
constexpr int BL_QSLICE = PMD_SLIDING_QUANTILE_SLICE;   // outputs per wave of quantile_kernel

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename E>
union bl_vec {                        // 16 bytes of a frame: one load, or V elements one by one
  u32x4 q;
  E e[16 / sizeof(E)];
};

// V consecutive floats of a row from column c on: 16-byte stores when the row allows, else one by one below N
template <int V>
__device__ __forceinline__ void bl_store(float* __restrict__ row, long c, long N, bool vec, const float* v) {
  if (vec) {
#pragma unroll
    for (int q = 0; q < V / 4; ++q) {
      const f32x4 o = {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
      *reinterpret_cast<f32x4*>(row + c + 4 * q) = o;
    }
  } else {
#pragma unroll
    for (int t = 0; t < V; ++t)
      if (c + t < N) row[c + t] = v[t];
  }
}

// V consecutive floats of a row from column c on (cj: the clamped columns)
template <int V>
__device__ __forceinline__ void bl_load_f32(const float* __restrict__ row, long c, const long* cj, bool vec, float* v) {
  if (vec) {
#pragma unroll
    for (int q = 0; q < V / 4; ++q) {
      const f32x4 o = *reinterpret_cast<const f32x4*>(row + c + 4 * q);
      v[4 * q] = o.x, v[4 * q + 1] = o.y, v[4 * q + 2] = o.z, v[4 * q + 3] = o.w;
    }
  } else {
#pragma unroll
    for (int t = 0; t < V; ++t) v[t] = row[cj[t]];
  }
}

template <typename E>
__global__ __launch_bounds__(64 * BL_WAVES) void bin_means_kernel(const E* __restrict__ Y, long ldy, int n, long N, int bin,
                                                                   int shift, int slice, float* __restrict__ K, long ldk,
                                                                   int vec_in, int vec_out) {
#pragma clang fp contract(off)
  constexpr int V = 16 / sizeof(E);
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long c = ((long)blockIdx.x * 64 + lane) * V;   // first pixel of this lane
  const int fa = ((int)blockIdx.y * BL_WAVES + w) * slice, fb = min(n, fa + slice);
  if (fa >= n || c >= N) return;
  const bool in_vec = vec_in && c + V <= N, out_vec = vec_out && c + V <= N;
  long cj[V];
#pragma unroll
  for (int t = 0; t < V; ++t) cj[t] = c + t < N ? c + t : N - 1;
  const int bmask = bin - 1;
  float bs[V];
#pragma unroll
  for (int t = 0; t < V; ++t) bs[t] = 0.f;

  for (int fs = fa; fs < fb; fs += BL_U) {
    bl_vec<E> y[BL_U];
#pragma unroll
    for (int u = 0; u < BL_U; ++u) {
      const E* row = Y + (long)min(fs + u, fb - 1) * ldy;   // past the slice: re-read its last frame, not used
      if (in_vec) {
        y[u].q = *reinterpret_cast<const u32x4*>(row + c);
      } else {
#pragma unroll
        for (int t = 0; t < V; ++t) y[u].e[t] = row[cj[t]];
      }
    }
#pragma unroll
    for (int u = 0; u < BL_U; ++u) {
      const int f = fs + u;
      if (f < fb) {                    // the same in every lane
        const int k = f & bmask;       // position of the frame in its bin
#pragma unroll
        for (int t = 0; t < V; ++t) bs[t] = k == 0 ? (float)y[u].e[t] : bs[t] + (float)y[u].e[t];
        if (k == bmask || f == n - 1) {
          float v[V];
          const float cnt = (float)(k + 1);
#pragma unroll
          for (int t = 0; t < V; ++t) v[t] = bin == 1 ? bs[t] : bs[t] / cnt;
          bl_store<V>(K + (long)(f >> shift) * ldk, c, N, out_vec, v);
        }
      }
    }
  }
}

template <bool MAX>
__device__ __forceinline__ float bl_ext(float a, float b) {
  return MAX ? __builtin_fmaxf(a, b) : __builtin_fminf(a, b);
}

template <bool MAX>
__global__ __launch_bounds__(64 * BL_WAVES) void extremum_kernel(const float* __restrict__ X, long ldx, long n, long N,
                                                                  long half, float* __restrict__ out, long ldo,
                                                                  float* __restrict__ work, long ldw, int vec_x,
                                                                  int vec_out, int vec_work) {
  constexpr int V = 4;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long c = ((long)blockIdx.y * 64 + lane) * V;
  const long W = 2 * half + 1;
  const long j0 = ((long)blockIdx.x * BL_WAVES + w) * W;     // first output of this wave's segment
  if (j0 >= n || c >= N) return;
  const bool full = c + V <= N;
  const bool xv = vec_x && full, ov = vec_out && full, wv = vec_work && full;
  long cj[V];
#pragma unroll
  for (int t = 0; t < V; ++t) cj[t] = c + t < N ? c + t : N - 1;
  const long rmax = min(W - 1, n - 1 - j0);                  // outputs j0 .. j0 + rmax
  const float none = __builtin_nanf("");
  float acc[V], v[V], b[V];

  // backward from frame min(j0 + half, n - 1) down to j0 - half; frames below 0 are padding
#pragma unroll
  for (int t = 0; t < V; ++t) acc[t] = none;
#pragma unroll 4
  for (long r = min(W - 1, n - 1 - j0 + half); r >= 0; --r) {
    const long f = j0 + r - half;
    bl_load_f32<V>(X + max(f, 0L) * ldx, c, cj, xv, v);
    if (f >= 0) {
#pragma unroll
      for (int t = 0; t < V; ++t) acc[t] = bl_ext<MAX>(acc[t], v[t]);
    }
    if (r <= rmax) bl_store<V>(work + (j0 + r) * ldw, c, N, wv, acc);
  }
  // forward from frame j0 + half up; frames from n on are padding
#pragma unroll
  for (int t = 0; t < V; ++t) acc[t] = none;
#pragma unroll 4
  for (long r = 0; r <= rmax; ++r) {
    const long f = j0 + r + half;
    bl_load_f32<V>(X + min(f, n - 1) * ldx, c, cj, xv, v);
    bl_load_f32<V>(work + (j0 + r) * ldw, c, cj, wv, b);
    if (f < n) {
#pragma unroll
      for (int t = 0; t < V; ++t) acc[t] = bl_ext<MAX>(acc[t], v[t]);
    }
#pragma unroll
    for (int t = 0; t < V; ++t) b[t] = bl_ext<MAX>(b[t], acc[t]);
    bl_store<V>(out + (j0 + r) * ldo, c, N, ov, b);
  }
}

// the order-preserving key of pmd_pixel_hist_accumulate: -0 before +0, every NaN last
__device__ __forceinline__ unsigned bl_key(float v) {
  const unsigned b = __float_as_uint(v);
  return v != v ? 0xFFFFFFFFu : b ^ ((unsigned)((int)b >> 31) | 0x80000000u);
}

__device__ __forceinline__ float bl_unkey(unsigned k) {
  return __uint_as_float(k & 0x80000000u ? k ^ 0x80000000u : ~k);
}

// The members of the window of output j, as keys: the rows max(0, j - half) .. min(n - 1, j + half) once each, then the
// copies that replicate the edges, row 0 another max(0, half - j) times and row n - 1 another max(0, j + half - (n - 1))
// times, as one visit with a multiplicity each.  visit(k, m): the V keys of a row, counted m times.
template <int V, typename F>
__device__ __forceinline__ void bl_window(const float* __restrict__ X, long ldx, long n, long half, long j, long c,
                                          const long* cj, bool xv, F&& visit) {
  const long lo = max(j - half, 0L), hi = min(j + half, n - 1);
  float v[V];
  unsigned k[V];
#pragma unroll 4                       // 8 rows in flight measured slower: 78 ms against 53 ms on 625 x 262 144 knots
  for (long r = lo; r <= hi; ++r) {
    bl_load_f32<V>(X + r * ldx, c, cj, xv, v);
#pragma unroll
    for (int t = 0; t < V; ++t) k[t] = bl_key(v[t]);
    visit(k, 1u);
  }
  const unsigned m0 = (unsigned)max(half - j, 0L), m1 = (unsigned)max(j + half - (n - 1), 0L);   // half < 2^30
  if (m0) {
    bl_load_f32<V>(X, c, cj, xv, v);
#pragma unroll
    for (int t = 0; t < V; ++t) k[t] = bl_key(v[t]);
    visit(k, m0);
  }
  if (m1) {
    bl_load_f32<V>(X + (n - 1) * ldx, c, cj, xv, v);
#pragma unroll
    for (int t = 0; t < V; ++t) k[t] = bl_key(v[t]);
    visit(k, m1);
  }
}

__global__ __launch_bounds__(64 * BL_WAVES) void quantile_kernel(const float* __restrict__ X, long ldx, long n, long N,
                                                                  long half, unsigned rank, float* __restrict__ out,
                                                                  long ldo, int vec_x, int vec_out) {
  constexpr int V = 4;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long c = ((long)blockIdx.y * 64 + lane) * V;
  const long j0 = ((long)blockIdx.x * BL_WAVES + w) * BL_QSLICE;   // first output of this wave's slice
  if (j0 >= n || c >= N) return;
  const long j1 = min(n, j0 + BL_QSLICE);
  const bool full = c + V <= N;
  const bool xv = vec_x && full, ov = vec_out && full;
  long cj[V];
#pragma unroll
  for (int t = 0; t < V; ++t) cj[t] = c + t < N ? c + t : N - 1;
  // per column: the answer key a of the current window, cl = #{key < a} and ce = #{key == a} of its members
  unsigned a[V], cl[V], ce[V];
  float v[V], o[V];

  // the first output: the smallest a with #{key <= a} > rank, bit by bit from the top
#pragma unroll
  for (int t = 0; t < V; ++t) a[t] = 0u;
  for (int b = 31; b >= 0; --b) {
    unsigned probe[V], cnt[V];
#pragma unroll
    for (int t = 0; t < V; ++t) probe[t] = a[t] | ((1u << b) - 1u), cnt[t] = 0u;
    bl_window<V>(X, ldx, n, half, j0, c, cj, xv, [&](const unsigned* k, unsigned m) {
#pragma unroll
      for (int t = 0; t < V; ++t) cnt[t] += k[t] <= probe[t] ? m : 0u;
    });
#pragma unroll
    for (int t = 0; t < V; ++t)
      if (cnt[t] <= rank) a[t] |= 1u << b;
  }
#pragma unroll
  for (int t = 0; t < V; ++t) cl[t] = ce[t] = 0u;
  bl_window<V>(X, ldx, n, half, j0, c, cj, xv, [&](const unsigned* k, unsigned m) {
#pragma unroll
    for (int t = 0; t < V; ++t) cl[t] += k[t] < a[t] ? m : 0u, ce[t] += k[t] == a[t] ? m : 0u;
  });
#pragma unroll
  for (int t = 0; t < V; ++t) o[t] = bl_unkey(a[t]);
  bl_store<V>(out + j0 * ldo, c, N, ov, o);

  for (long j = j0 + 1; j < j1; ++j) {
    // the window loses the member at j - 1 - half and gains the one at j + half, both clamped
    unsigned ko[V], ki[V];
    bl_load_f32<V>(X + min(max(j - 1 - half, 0L), n - 1) * ldx, c, cj, xv, v);
#pragma unroll
    for (int t = 0; t < V; ++t) ko[t] = bl_key(v[t]);
    bl_load_f32<V>(X + min(j + half, n - 1) * ldx, c, cj, xv, v);
#pragma unroll
    for (int t = 0; t < V; ++t) ki[t] = bl_key(v[t]);
    bool stale = false;
#pragma unroll
    for (int t = 0; t < V; ++t) {
      cl[t] += (ki[t] < a[t] ? 1u : 0u) - (ko[t] < a[t] ? 1u : 0u);
      ce[t] += (ki[t] == a[t] ? 1u : 0u) - (ko[t] == a[t] ? 1u : 0u);
      stale |= rank < cl[t] || rank - cl[t] >= ce[t];
    }
    if (__any(stale)) {                // the same in every lane of the wave
      // the neighbours of a among the members: the largest key below with its count, the smallest above with its count
      unsigned lo[V], nlo[V], hi[V], nhi[V];
#pragma unroll
      for (int t = 0; t < V; ++t) lo[t] = 0u, hi[t] = 0xFFFFFFFFu, nlo[t] = nhi[t] = 0u;
      bl_window<V>(X, ldx, n, half, j, c, cj, xv, [&](const unsigned* k, unsigned m) {
#pragma unroll
        for (int t = 0; t < V; ++t) {
          if (k[t] < a[t]) {
            nlo[t] = k[t] > lo[t] ? m : (k[t] == lo[t] ? nlo[t] + m : nlo[t]);
            lo[t] = k[t] > lo[t] ? k[t] : lo[t];
          } else if (k[t] > a[t]) {
            nhi[t] = k[t] < hi[t] ? m : (k[t] == hi[t] ? nhi[t] + m : nhi[t]);
            hi[t] = k[t] < hi[t] ? k[t] : hi[t];
          }
        }
      });
      // one member was replaced, so the answer moves by one distinct value: down with cl == rank + 1, or up with
      // cl + ce == rank
#pragma unroll
      for (int t = 0; t < V; ++t) {
        if (rank < cl[t]) {
          a[t] = lo[t], ce[t] = nlo[t], cl[t] -= nlo[t];
        } else if (rank - cl[t] >= ce[t]) {
          cl[t] += ce[t], a[t] = hi[t], ce[t] = nhi[t];
        }
      }
    }
#pragma unroll
    for (int t = 0; t < V; ++t) o[t] = bl_unkey(a[t]);
    bl_store<V>(out + j * ldo, c, N, ov, o);
  }
}

template <typename E, int MODE>
__global__ __launch_bounds__(64 * BL_WAVES) void apply_kernel(const E* __restrict__ X, long ldx, int n, long N, int f0, int T,
                                                               int bin, int shift, int nb, const float* __restrict__ K,
                                                               long ldk, float min_baseline, float* __restrict__ out,
                                                               long ldo, int vec_x, int vec_k, int vec_out) {
#pragma clang fp contract(off)
  constexpr int V = 16 / sizeof(E);
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long c = ((long)blockIdx.x * 64 + lane) * V;
  const int fa = ((int)blockIdx.y * BL_WAVES + w) * BL_APPLY_SLICE, fb = min(n, fa + BL_APPLY_SLICE);
  if (fa >= n || c >= N) return;
  const bool full = c + V <= N;
  const bool xv = vec_x && full, kv = vec_k && full, ov = vec_out && full;
  long cj[V];
#pragma unroll
  for (int t = 0; t < V; ++t) cj[t] = c + t < N ? c + t : N - 1;
  float ka[V], kb[V];
  int ra = -1, rb = -1;                // the knot rows in ka and kb
#pragma unroll
  for (int t = 0; t < V; ++t) ka[t] = kb[t] = 0.f;

  for (int fs = fa; fs < fb; fs += BL_U) {
    bl_vec<E> y[BL_U];
    if (MODE != 0) {
#pragma unroll
      for (int u = 0; u < BL_U; ++u) {
        const E* row = X + (long)min(fs + u, fb - 1) * ldx;   // past the slice: re-read its last frame, not used
        if (xv) {
          y[u].q = *reinterpret_cast<const u32x4*>(row + c);
        } else {
#pragma unroll
          for (int t = 0; t < V; ++t) y[u].e[t] = row[cj[t]];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < BL_U; ++u) {
      const int f = fs + u;
      if (f < fb) {                    // the same in every lane, as is everything up to the knot rows
        // twice the frame and twice the centres: integers
        const int t2 = 2 * (f0 + f), jt = (f0 + f) >> shift;
        const int cc2 = 2 * jt * bin + min(bin, T - jt * bin) - 1;
        const int j = t2 >= cc2 ? jt : jt - 1;              // the last bin whose centre is at or before the frame
        int ja, jb;
        bool exact = true;
        float wt = 0.f;
        if (j < 0) {
          ja = jb = 0;
        } else if (j >= nb - 1) {
          ja = jb = nb - 1;
        } else {
          const int c2 = 2 * j * bin + bin - 1;
          const int n2 = 2 * (j + 1) * bin + min(bin, T - (j + 1) * bin) - 1;
          ja = j, jb = j + 1;
          exact = t2 == c2;
          wt = (0.5f * (float)(t2 - c2)) / (0.5f * (float)(n2 - c2));
        }
        if (ja != ra) {
          if (ja == rb) {
#pragma unroll
            for (int t = 0; t < V; ++t) ka[t] = kb[t];
          } else {
            bl_load_f32<V>(K + (long)ja * ldk, c, cj, kv, ka);
          }
          ra = ja;
        }
        if (jb != rb) {
          if (jb == ra) {
#pragma unroll
            for (int t = 0; t < V; ++t) kb[t] = ka[t];
          } else {
            bl_load_f32<V>(K + (long)jb * ldk, c, cj, kv, kb);
          }
          rb = jb;
        }
        float o[V];
#pragma unroll
        for (int t = 0; t < V; ++t) {
          const float d = kb[t] - ka[t];
          const float base = exact ? ka[t] : ka[t] + wt * d;
          if (MODE == 0) {
            o[t] = base;
          } else {
            const float r = (float)y[u].e[t] - base;
            o[t] = MODE == 1 ? r : (base > min_baseline ? r / base : 0.f);
          }
        }
        bl_store<V>(out + (long)f * ldo, c, N, ov, o);
      }
    }
  }
}

template <typename E>
void launch_apply(pmd_ctx* ctx, const void* X, long ldx, int n, long N, int f0, int T, int bin, int shift, int nb,
                  const float* K, long ldk, int mode, float min_baseline, float* out, long ldo) {
  constexpr int V = 16 / sizeof(E);
  const int slices = (n + BL_APPLY_SLICE - 1) / BL_APPLY_SLICE;
  const dim3 grid((unsigned)((N + 64 * V - 1) / (64 * V)), (unsigned)((slices + BL_WAVES - 1) / BL_WAVES));
  const dim3 block(64 * BL_WAVES);
  const int vec_x = X && (ldx * sizeof(E)) % 16 == 0 && (uintptr_t)X % 16 == 0;
  const int vec_k = (ldk * 4) % 16 == 0 && (uintptr_t)K % 16 == 0;
  const int vec_out = (ldo * 4) % 16 == 0 && (uintptr_t)out % 16 == 0;
  const E* x = (const E*)X;
  if (mode == 0)
    hipLaunchKernelGGL((apply_kernel<E, 0>), grid, block, 0, ctx->stream, x, ldx, n, N, f0, T, bin, shift, nb, K, ldk,
                       min_baseline, out, ldo, vec_x, vec_k, vec_out);
  else if (mode == 1)
    hipLaunchKernelGGL((apply_kernel<E, 1>), grid, block, 0, ctx->stream, x, ldx, n, N, f0, T, bin, shift, nb, K, ldk,
                       min_baseline, out, ldo, vec_x, vec_k, vec_out);
  else
    hipLaunchKernelGGL((apply_kernel<E, 2>), grid, block, 0, ctx->stream, x, ldx, n, N, f0, T, bin, shift, nb, K, ldk,
                       min_baseline, out, ldo, vec_x, vec_k, vec_out);
}

template <typename E>
void launch_bins(pmd_ctx* ctx, const void* Y, long ldy, int n, long N, int bin, int shift, float* K, long ldk) {
  constexpr int V = 16 / sizeof(E);
  const int slice = bin > BL_MIN_SLICE ? bin : BL_MIN_SLICE;
  const int slices = (n + slice - 1) / slice;
  const dim3 grid((unsigned)((N + 64 * V - 1) / (64 * V)), (unsigned)((slices + BL_WAVES - 1) / BL_WAVES));
  const dim3 block(64 * BL_WAVES);
  const int vec_in = (ldy * sizeof(E)) % 16 == 0 && (uintptr_t)Y % 16 == 0;
  const int vec_out = (ldk * 4) % 16 == 0 && (uintptr_t)K % 16 == 0;
  hipLaunchKernelGGL(bin_means_kernel<E>, grid, block, 0, ctx->stream, (const E*)Y, ldy, n, N, bin, shift, slice, K, ldk,
                     vec_in, vec_out);
}

bool bl_bad_bin(int bin) { return bin < 1 || bin > PMD_BASELINE_MAX_BIN || (bin & (bin - 1)) != 0; }

int bl_shift(int bin) {
  int s = 0;
  while ((1 << s) < bin) ++s;
  return s;
}

}  // namespace

extern "C" {

int pmd_bin_means(pmd_ctx* ctx, const void* Y, int elem, long ldy, int n, long N, long f0, int bin, float* K, long ldk) {
  CTX_CHECK(ctx);
  const char* what = "pmd_bin_means";
  if (n < 1 || n > PMD_STATS_BLOCK) return pmd_fail(ctx, PMD_ERR_ARG, what, "n outside 1 .. PMD_STATS_BLOCK");
  if (N < 1 || ldy < N || ldk < N) return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (N >= 1, ldy >= N, ldk >= N)");
  if (bl_bad_bin(bin)) return pmd_fail(ctx, PMD_ERR_ARG, what, "bin is not a power of two in 1 .. PMD_BASELINE_MAX_BIN");
  if (f0 < 0 || f0 % bin != 0 || f0 + n >= 0x80000000L)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "f0 is negative, not a multiple of bin, or f0 + n >= 2^31");
  if (pmd_bad_elem(elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown element type");
  if (!Y || !K) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if ((N + 255) / 256 > 0x7fffffffL) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many pixels in one call");
  pmd_prof_scope prof__(ctx, "bin_means");
  float* k0 = K + f0 / bin * ldk;      // the block's first knot row
  const int shift = bl_shift(bin);
  pmd_with_elem(elem, [&](auto e) { launch_bins<typename decltype(e)::type>(ctx, Y, ldy, n, N, bin, shift, k0, ldk); });
  PMD_LAUNCH_CHECK(ctx, "bin_means_kernel");
  return PMD_OK;
}

long pmd_sliding_extremum_work_floats(long n, long Nc) { return n < 1 || Nc < 1 ? 0 : n * pmd_round_up(Nc, 4); }

int pmd_sliding_extremum(pmd_ctx* ctx, const float* X, long ldx, long n, long N, long half, int is_max, float* out, long ldo,
                         float* work, long work_floats) {
  CTX_CHECK(ctx);
  const char* what = "pmd_sliding_extremum";
  if (n < 1 || N < 1 || ldx < N || ldo < N)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (n >= 1, N >= 1, ldx >= N, ldo >= N)");
  if (n > 0x7fffffffL) return pmd_fail(ctx, PMD_ERR_ARG, what, "n >= 2^31");
  if (half < 0) return pmd_fail(ctx, PMD_ERR_ARG, what, "half is negative");
  if (is_max != 0 && is_max != 1) return pmd_fail(ctx, PMD_ERR_ARG, what, "is_max is neither 0 nor 1");
  if (!X || !out || !work) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if (work_floats < pmd_sliding_extremum_work_floats(n, N))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "workspace smaller than pmd_sliding_extremum_work_floats(n, N)");
  const float *xe = X + (n - 1) * ldx + N, *oe = out + (n - 1) * ldo + N;
  if ((uintptr_t)X < (uintptr_t)oe && (uintptr_t)out < (uintptr_t)xe)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "X and out overlap");
  if ((N + 255) / 256 > 65535) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many pixels in one call");
  // a window of half >= n - 1 holds every frame: the same result, and W stays below 2 n
  const long h = half < n - 1 ? half : n - 1;
  const long W = 2 * h + 1, segments = (n + W - 1) / W;
  pmd_prof_scope prof__(ctx, "sliding_extremum");
  const long ldw = pmd_round_up(N, 4);
  const dim3 grid((unsigned)((segments + BL_WAVES - 1) / BL_WAVES), (unsigned)((N + 255) / 256)), block(64 * BL_WAVES);
  const int vec_x = (ldx * 4) % 16 == 0 && (uintptr_t)X % 16 == 0;
  const int vec_out = (ldo * 4) % 16 == 0 && (uintptr_t)out % 16 == 0;
  const int vec_work = (uintptr_t)work % 16 == 0;
  if (is_max)
    hipLaunchKernelGGL(extremum_kernel<true>, grid, block, 0, ctx->stream, X, ldx, n, N, h, out, ldo, work, ldw, vec_x,
                       vec_out, vec_work);
  else
    hipLaunchKernelGGL(extremum_kernel<false>, grid, block, 0, ctx->stream, X, ldx, n, N, h, out, ldo, work, ldw, vec_x,
                       vec_out, vec_work);
  PMD_LAUNCH_CHECK(ctx, "extremum_kernel");
  return PMD_OK;
}

long pmd_sliding_quantile_work_floats(long n, long Nc, long half) {
  (void)n, (void)Nc, (void)half;       // the state of a column lives in registers
  return 0;
}

int pmd_sliding_quantile(pmd_ctx* ctx, const float* X, long ldx, long n, long N, long half, long rank, float* out, long ldo,
                         float* work, long work_floats) {
  CTX_CHECK(ctx);
  const char* what = "pmd_sliding_quantile";
  if (n < 1 || N < 1 || ldx < N || ldo < N)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (n >= 1, N >= 1, ldx >= N, ldo >= N)");
  if (n > 0x7fffffffL) return pmd_fail(ctx, PMD_ERR_ARG, what, "n >= 2^31");
  if (half < 0 || half >= (1L << 30)) return pmd_fail(ctx, PMD_ERR_ARG, what, "half outside 0 .. 2^30 - 1");
  if (rank < 0 || rank > 2 * half) return pmd_fail(ctx, PMD_ERR_ARG, what, "rank outside 0 .. 2 half");
  if (!X || !out) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  const long need = pmd_sliding_quantile_work_floats(n, N, half);
  if (work_floats < need || (need > 0 && !work))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "workspace smaller than pmd_sliding_quantile_work_floats(n, N, half)");
  const float *xe = X + (n - 1) * ldx + N, *oe = out + (n - 1) * ldo + N;
  if ((uintptr_t)X < (uintptr_t)oe && (uintptr_t)out < (uintptr_t)xe)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "X and out overlap");
  if ((N + 255) / 256 > 65535) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many pixels in one call");
  pmd_prof_scope prof__(ctx, "sliding_quantile");
  const long slices = (n + BL_QSLICE - 1) / BL_QSLICE;
  const dim3 grid((unsigned)((slices + BL_WAVES - 1) / BL_WAVES), (unsigned)((N + 255) / 256)), block(64 * BL_WAVES);
  const int vec_x = (ldx * 4) % 16 == 0 && (uintptr_t)X % 16 == 0;
  const int vec_out = (ldo * 4) % 16 == 0 && (uintptr_t)out % 16 == 0;
  hipLaunchKernelGGL(quantile_kernel, grid, block, 0, ctx->stream, X, ldx, n, N, half, (unsigned)rank, out, ldo, vec_x,
                     vec_out);
  PMD_LAUNCH_CHECK(ctx, "quantile_kernel");
  return PMD_OK;
}

int pmd_baseline_apply(pmd_ctx* ctx, const void* X, int elem, long ldx, int n, long N, long f0, long T, int bin,
                       const float* K, long ldk, int mode, float min_baseline, float* out, long ldo) {
  CTX_CHECK(ctx);
  const char* what = "pmd_baseline_apply";
  if (n < 1 || n > PMD_STATS_BLOCK) return pmd_fail(ctx, PMD_ERR_ARG, what, "n outside 1 .. PMD_STATS_BLOCK");
  if (mode < 0 || mode > 2) return pmd_fail(ctx, PMD_ERR_ARG, what, "mode outside 0 .. 2");
  if (N < 1 || ldk < N || ldo < N || (X && ldx < N))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (N >= 1, ldx >= N, ldk >= N, ldo >= N)");
  if (bl_bad_bin(bin)) return pmd_fail(ctx, PMD_ERR_ARG, what, "bin is not a power of two in 1 .. PMD_BASELINE_MAX_BIN");
  if (T < 1 || T >= PMD_BASELINE_MAX_FRAMES) return pmd_fail(ctx, PMD_ERR_ARG, what, "T outside 1 .. 2^23 - 1");
  if (f0 < 0 || f0 + n > T) return pmd_fail(ctx, PMD_ERR_ARG, what, "frames f0 .. f0 + n lie outside 0 .. T");
  if (pmd_bad_elem(elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown element type");
  if (!K || !out || (!X && mode != 0)) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if ((N + 255) / 256 > 0x7fffffffL) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many pixels in one call");
  pmd_prof_scope prof__(ctx, "baseline_apply");
  const int shift = bl_shift(bin), nb = (int)((T + bin - 1) / bin);
  if (mode == 0 || elem == PMD_ELEM_F32)   // mode 0 reads no X: one instantiation serves every element type
    launch_apply<float>(ctx, mode == 0 ? nullptr : X, ldx, n, N, (int)f0, (int)T, bin, shift, nb, K, ldk, mode,
                        min_baseline, out, ldo);
  else if (elem == PMD_ELEM_U16)
    launch_apply<uint16_t>(ctx, X, ldx, n, N, (int)f0, (int)T, bin, shift, nb, K, ldk, mode, min_baseline, out, ldo);
  else
    launch_apply<int16_t>(ctx, X, ldx, n, N, (int)f0, (int)T, bin, shift, nb, K, ldk, mode, min_baseline, out, ldo);
  PMD_LAUNCH_CHECK(ctx, "apply_kernel");
  return PMD_OK;
}

}  // extern "C"
