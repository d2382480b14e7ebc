// Superpixel seeds (localmd_amd/superpixels.py): the neighbour moments of the thresholded movie, and the connected
// components of a per-edge pixel graph.
//
// pmd_threshold_moments_accumulate.  y[f][c] = v > thr[c] ? fl32(v - thr[c]) : 0 with v = (float) Y[f][c]; per pixel six
// fp64 sums over the frames: y, y^2 and y_p y_q for the forward neighbours E (0,+1), SW (+1,-1), S (+1,0), SE (+1,+1); a
// neighbour outside the image counts as 0.  4 (2) bytes per pixel and frame against 12 fp64 operations and 5 widenings;
// measured, the fp64 arithmetic and not the memory bounds it.
//
// Lanes run along j.  A wave covers 64 consecutive columns of TM_ROWS + 1 rows and owns the pixels of lanes 1 .. 62 in the
// first TM_ROWS of them: lane 0 is the west halo (it supplies SW of lane 1), lane 63 the east halo (E and SE of lane 62),
// and the last row is the south halo, which the wave below owns and loads as well (that second load is a cache hit: the
// movie comes from HBM about once, (TM_ROWS + 1) / TM_ROWS x 64 / 62 of it from the caches).  Every lane rectifies the
// elements it loaded against the thresholds of its own column, which it holds in registers for the whole call, halo or
// not: the rectified value of a pixel is formed by the same two operations wherever it is needed, so no seam can see
// another value of it.  E, SW and SE come from the adjacent lanes by DPP moves, S from the lane's own next row.
//
// Order of the arithmetic: every product is (double) a * (double) b of two fp32 values, exact; every sum is one fp64
// chain per pixel over the frames in ascending order, started from the value stored in mom and stored back once.  The
// loads of TM_U frames are issued before their use; the six chains of a pixel are independent.  The bits of pixel c depend
// on the columns of c and its forward neighbours, their thresholds and the stored state only: not on how the frames are
// split over calls, on ldy, on the element type holding the same values, or on where the pixel lies in a tile.  One owner
// per pixel: no atomics, no LDS, no workspace, no synchronisation.
//
// pmd_grid_components.  label[c] = the smallest pixel index of c's component in the graph whose edges are the bits of
// edges[c] (bit 0 E, 1 SW, 2 S, 3 SE; a bit that points outside the image is ignored).  Union-find with the smaller index
// as parent, three launches; the kernel boundaries are the only device-wide synchronisation, no workgroup waits for
// another:
//   cc_tiles_kernel    a workgroup labels a 16 x 64 tile in LDS (edges inside the tile only) and writes every pixel's
//                      tile root, as a global pixel index, to label;
//   cc_merge_kernel    a thread per pixel joins the edges that cross a tile border on label, the global parent array;
//   cc_flatten_kernel  label[c] = root of c.
// See the comment above cc_union for why the result does not depend on which thread wins a race and why it terminates.
#include "pmd_common.h"
#include "../../include/pmd_hip.h"

namespace {

// ---- threshold moments ---------------------------------------------------------------------------------------------
constexpr int TM_ROWS = 2;            // pixel rows a lane owns
constexpr int TM_WAVES = 4;           // waves of a workgroup, stacked along i
constexpr int TM_COLS = 62;           // columns a wave owns: lanes 1 .. 62
constexpr int TM_U = 8;               // frames whose loads are in flight per lane

// The value of the lane to the left / to the right, by one DPP move across the whole wave (no LDS traffic).  Lane 0 of
// from_left and lane 63 of from_right get 0; neither owns a pixel that would use it.
__device__ __forceinline__ float from_left(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x138, 0xf, 0xf, false));   // wave_shr:1
}
__device__ __forceinline__ float from_right(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x130, 0xf, 0xf, false));   // wave_shl:1
}

template <typename E>
__global__ __launch_bounds__(64 * TM_WAVES) void threshold_moments_kernel(const E* __restrict__ Y, long ldy, int n, int d1,
                                                                         int d2, const float* __restrict__ thr,
                                                                         double* __restrict__ mom) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i0 = ((int)blockIdx.x * TM_WAVES + w) * TM_ROWS;
  if (i0 >= d1) return;                // the whole wave: nothing below uses a workgroup barrier
  const int j = (int)blockIdx.y * TM_COLS + lane - 1;
  const bool jin = j >= 0 && j < d2;
  const int jc = min(max(j, 0), d2 - 1);
  const long D = (long)d1 * d2;
  long off[TM_ROWS + 1];               // clamped: every load is inside the frame; what lies outside the image counts as 0
  bool in[TM_ROWS + 1];
  float t[TM_ROWS + 1];
#pragma unroll
  for (int r = 0; r <= TM_ROWS; ++r) {
    in[r] = jin && i0 + r < d1;
    off[r] = (long)min(i0 + r, d1 - 1) * d2 + jc;
    t[r] = thr[off[r]];
  }
  const bool mine = jin && lane >= 1 && lane <= TM_COLS;
  double acc[TM_ROWS][6];
#pragma unroll
  for (int r = 0; r < TM_ROWS; ++r)
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[r][k] = mine && in[r] ? mom[k * D + off[r]] : 0.0;

  for (int fs = 0; fs < n; fs += TM_U) {
    E v[TM_U][TM_ROWS + 1];
#pragma unroll
    for (int u = 0; u < TM_U; ++u) {
      const E* frame = Y + (long)min(fs + u, n - 1) * ldy;   // past the end: re-read the last frame, not used
#pragma unroll
      for (int r = 0; r <= TM_ROWS; ++r) v[u][r] = frame[off[r]];
    }
#pragma unroll
    for (int u = 0; u < TM_U; ++u) {
      if (fs + u < n) {                // the same in every lane
        float y[TM_ROWS + 1], ye[TM_ROWS + 1], yw[TM_ROWS + 1];
#pragma unroll
        for (int r = 0; r <= TM_ROWS; ++r) {
          const float x = (float)v[u][r];
          y[r] = in[r] && x > t[r] ? x - t[r] : 0.f;        // a NaN value or threshold compares false
        }
#pragma unroll
        for (int r = 0; r <= TM_ROWS; ++r) {
          ye[r] = from_right(y[r]);                          // column j + 1 (lane 63 owns nothing)
          yw[r] = from_left(y[r]);                           // column j - 1 (lane 0 owns nothing)
        }
#pragma unroll
        for (int r = 0; r < TM_ROWS; ++r) {
          const double a = (double)y[r];                     // the products are exact, so a fused multiply-add rounds
          acc[r][0] = acc[r][0] + a;                         // as the product followed by the sum does
          acc[r][1] = __builtin_fma(a, a, acc[r][1]);
          acc[r][2] = __builtin_fma(a, (double)ye[r], acc[r][2]);
          acc[r][3] = __builtin_fma(a, (double)yw[r + 1], acc[r][3]);
          acc[r][4] = __builtin_fma(a, (double)y[r + 1], acc[r][4]);
          acc[r][5] = __builtin_fma(a, (double)ye[r + 1], acc[r][5]);
        }
      }
    }
  }

#pragma unroll
  for (int r = 0; r < TM_ROWS; ++r)
    if (mine && in[r])
#pragma unroll
      for (int k = 0; k < 6; ++k) mom[k * D + off[r]] = acc[r][k];
}

template <typename E>
void launch_moments(pmd_ctx* ctx, const void* Y, long ldy, int n, int d1, int d2, const float* thr, double* mom) {
  const dim3 grid((unsigned)((d1 + TM_WAVES * TM_ROWS - 1) / (TM_WAVES * TM_ROWS)), (unsigned)((d2 + TM_COLS - 1) / TM_COLS));
  hipLaunchKernelGGL((threshold_moments_kernel<E>), grid, dim3(64 * TM_WAVES), 0, ctx->stream, (const E*)Y, ldy, n, d1, d2,
                     thr, mom);
}

// ---- connected components ------------------------------------------------------------------------------------------
constexpr int CC_TH = 16, CC_TW = 64;                        // a tile: 1024 pixels, 4 KB of parents in LDS
constexpr int CC_THREADS = 256;
constexpr int CC_WG = __HIP_MEMORY_SCOPE_WORKGROUP, CC_AGENT = __HIP_MEMORY_SCOPE_AGENT;

// The forward neighbour of bit b: (di, dj) = E (0, +1), SW (+1, -1), S (+1, 0), SE (+1, +1).
__device__ __forceinline__ int cc_di(int b) { return b != 0; }
__device__ __forceinline__ int cc_dj(int b) { return b == 0 ? 1 : b - 2; }

// The parent array P obeys, at every moment and for every element x: P[x] <= x, and P[x] lies in the component of x
// (first invariant); it changes by fetch_min only, so a parent is only ever lowered (second).  Every access is a relaxed
// atomic of scope SCOPE (workgroup on the LDS array of a tile, agent on the global array, whose writers may sit on
// another XCD: a plain load could be served from a stale L1 line).  A value read is therefore a value P[x] once held,
// which by the two invariants is an ancestor of x or x itself; the newest value only names a lower ancestor.
//
// cc_find walks to a self-parent.  x strictly decreases on every step, so it ends after at most x steps whatever it
// reads; the root it returns may have been hooked since, which cc_union repairs.
template <int SCOPE>
__device__ __forceinline__ int cc_find(int* P, int x) {
  for (;;) {
    const int p = __hip_atomic_load(P + x, __ATOMIC_RELAXED, SCOPE);
    if (p >= x) return x;              // p == x: a root (p > x never holds)
    x = p;
  }
}

// cc_union joins the components of a and b.  With a > b both (apparent) roots, fetch_min(P[a], b) returns old:
//   old == a  a was a root and now hangs under b: done.
//   old != a  another thread lowered P[a] to old < a first.  P[a] is now min(old, b): if that is b, a's link to old was
//             replaced by the link to b; either way joining old with b restores or completes the component, so the loop
//             goes on with a = old.  A failed exchange thus means someone else made progress, and a + b has strictly
//             decreased: the loop ends after fewer than a + b + 2 <= 2 D rounds whatever the other threads do.
// Termination needs no fairness and no waiting: a thread never spins on a value another thread has to write.  The result
// is race-free in the sense that matters: when all unions have returned, two pixels have the same root iff a path of
// edges joins them, and since parents only point downwards the root of a component is its smallest index, whichever
// thread won which exchange.  `limit` bounds the rounds all the same; false says it was reached (the caller raises the
// give-up flag and the entry point returns an error).
template <int SCOPE>
__device__ __forceinline__ bool cc_union(int* P, int a, int b, long limit) {
  for (long it = 0; it < limit; ++it) {
    a = cc_find<SCOPE>(P, a);
    b = cc_find<SCOPE>(P, b);
    if (a == b) return true;
    if (a < b) {
      const int s = a;
      a = b, b = s;
    }
    const int old = __hip_atomic_fetch_min(P + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) return true;
    a = old;
  }
  return false;
}

__global__ __launch_bounds__(CC_THREADS) void cc_tiles_kernel(const uint8_t* __restrict__ edges, int* __restrict__ label,
                                                              int d1, int d2, int ntx, int* flag) {
  __shared__ int P[CC_TH * CC_TW];
  const int i0 = (int)(blockIdx.x / ntx) * CC_TH, j0 = (int)(blockIdx.x % ntx) * CC_TW;
  for (int l = threadIdx.x; l < CC_TH * CC_TW; l += CC_THREADS) P[l] = l;
  __syncthreads();
  bool ok = true;
  for (int l = threadIdx.x; l < CC_TH * CC_TW; l += CC_THREADS) {
    const int li = l / CC_TW, lj = l % CC_TW;
    if (i0 + li >= d1 || j0 + lj >= d2) continue;
    const int e = edges[(long)(i0 + li) * d2 + j0 + lj];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int qi = li + cc_di(b), qj = lj + cc_dj(b);
      if (!((e >> b) & 1) || qi >= CC_TH || qj < 0 || qj >= CC_TW || i0 + qi >= d1 || j0 + qj >= d2) continue;
      ok = cc_union<CC_WG>(P, l, qi * CC_TW + qj, 2 * CC_TH * CC_TW) && ok;
    }
  }
  __syncthreads();
  // the local order is the global order restricted to the tile, so the smallest local index is the smallest global one
  for (int l = threadIdx.x; l < CC_TH * CC_TW; l += CC_THREADS) {
    const int li = l / CC_TW, lj = l % CC_TW;
    if (i0 + li >= d1 || j0 + lj >= d2) continue;
    const int r = cc_find<CC_WG>(P, l);
    label[(long)(i0 + li) * d2 + j0 + lj] = (i0 + r / CC_TW) * d2 + j0 + r % CC_TW;
  }
  if (!ok) __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, CC_AGENT);
}

__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(const uint8_t* __restrict__ edges, int* label, int d1, int d2,
                                                              int* flag) {
  const long D = (long)d1 * d2;
  const long c = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (c >= D) return;
  const int e = edges[c];
  if (!(e & 15)) return;
  const int i = (int)(c / d2), j = (int)(c % d2);
  bool ok = true;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int qi = i + cc_di(b), qj = j + cc_dj(b);
    if (!((e >> b) & 1) || qi >= d1 || qj < 0 || qj >= d2) continue;
    if (qi / CC_TH == i / CC_TH && qj / CC_TW == j / CC_TW) continue;      // joined in LDS already
    ok = cc_union<CC_AGENT>(label, (int)c, (int)((long)qi * d2 + qj), 2 * D + 2) && ok;
  }
  if (!ok) __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, CC_AGENT);
}

// No parent is lowered below a root any more; storing the root of c into label[c] keeps both invariants, so the walks
// of the other threads through label[c] stay valid.
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int* label, long D) {
  const long c = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (c >= D) return;
  __hip_atomic_store(label + c, cc_find<CC_AGENT>(label, (int)c), __ATOMIC_RELAXED, CC_AGENT);
}

}  // namespace

extern "C" {

int pmd_threshold_moments_accumulate(pmd_ctx* ctx, const void* Y, int elem, long ldy, int n, int d1, int d2,
                                     const float* thr, double* mom) {
  CTX_CHECK(ctx);
  const char* what = "pmd_threshold_moments_accumulate";
  if (n < 1 || d1 < 1 || d2 < 1) return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (n >= 1, d1 >= 1, d2 >= 1)");
  if (ldy < (long)d1 * d2) return pmd_fail(ctx, PMD_ERR_ARG, what, "ldy < d1 * d2");
  if (pmd_bad_elem(elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown element type");
  if (!Y || !thr || !mom) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if ((d2 + TM_COLS - 1) / TM_COLS > 65535) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many columns in one call");
  pmd_prof_scope prof__(ctx, "threshold_moments_accumulate");
  pmd_with_elem(elem, [&](auto e) { launch_moments<typename decltype(e)::type>(ctx, Y, ldy, n, d1, d2, thr, mom); });
  PMD_LAUNCH_CHECK(ctx, "threshold_moments_kernel");
  return PMD_OK;
}

size_t pmd_grid_components_workspace_bytes(int d1, int d2) { return d1 < 1 || d2 < 1 ? 0 : 256; }

int pmd_grid_components(pmd_ctx* ctx, int d1, int d2, const uint8_t* edges, int* label, void* ws, size_t ws_bytes) {
  CTX_CHECK(ctx);
  const char* what = "pmd_grid_components";
  if (d1 < 1 || d2 < 1) return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (d1 >= 1, d2 >= 1)");
  const long D = (long)d1 * d2;
  if (D >= 0x80000000L) return pmd_fail(ctx, PMD_ERR_ARG, what, "d1 * d2 >= 2^31");
  if (!edges || !label || !ws) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if (ws_bytes < pmd_grid_components_workspace_bytes(d1, d2)) return pmd_fail(ctx, PMD_ERR_WORKSPACE, what, "workspace too small");
  const int ntx = (d2 + CC_TW - 1) / CC_TW;
  const long tiles = (long)ntx * ((d1 + CC_TH - 1) / CC_TH);
  if (tiles > 0x7fffffffL) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many tiles");
  int* flag = (int*)ws;
  pmd_prof_scope prof__(ctx, "grid_components");
  PMD_HIP(ctx, hipMemsetAsync(flag, 0, 16, ctx->stream));
  const unsigned nblk = (unsigned)((D + CC_THREADS - 1) / CC_THREADS);
  hipLaunchKernelGGL(cc_tiles_kernel, dim3((unsigned)tiles), dim3(CC_THREADS), 0, ctx->stream, edges, label, d1, d2, ntx, flag);
  PMD_LAUNCH_CHECK(ctx, "cc_tiles_kernel");
  hipLaunchKernelGGL(cc_merge_kernel, dim3(nblk), dim3(CC_THREADS), 0, ctx->stream, edges, label, d1, d2, flag);
  PMD_LAUNCH_CHECK(ctx, "cc_merge_kernel");
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(nblk), dim3(CC_THREADS), 0, ctx->stream, label, D);
  PMD_LAUNCH_CHECK(ctx, "cc_flatten_kernel");
  int gave_up = 0;
  PMD_HIP(ctx, hipMemcpyAsync(&gave_up, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  PMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (gave_up) return pmd_fail(ctx, PMD_ERR_UNSUPPORTED, what, "a union gave up at its round limit; label is not valid");
  return PMD_OK;
}

}  // extern "C"
