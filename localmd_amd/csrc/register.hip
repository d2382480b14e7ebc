// Rigid motion correction by template matching (localmd_amd/register.py): the un-normalised zero-mean cross-correlation
// of every frame with the template's interior over all shifts |dy| <= my, |dx| <= mx (pmd_shift_correlate), the integer
// peak of every surface with its 3 x 3 neighbourhood (pmd_shift_peak), and the shifted, bilinearly interpolated movie
// (pmd_shift_apply).
//
// Geometry.  The window is rows [my, d1 - my) x columns [mx, d2 - mx) of the template, h x w pixels; t' is the template
// on it minus its mean (row-major, h x w).  With sy = dy + my and sx = dx + mx the surface is
//     C[sy, sx] = sum_{i < h, j < w} t'[i, j] f[i + sy, j + sx],
// every term inside the frame.
//
// correlate_kernel    vector FMAs out of a sliding register window.  A workgroup takes one frame and one RG_TH x RG_TW
//                     tile of the window; the (rows + 2 my) x (columns + 2 mx) halo of the frame is widened to fp32 into
//                     LDS once.  A lane owns one sy and a run of RG_R = 8 consecutive sx; for a window row it walks j in
//                     steps of four: one 16-byte LDS read brings the next four frame values into a 12-register window
//                     and feeds 32 FMAs, whose t'[i, j] operand is the same for the whole wave (a scalar load).  So an
//                     LDS read serves 32 FMAs of a lane and the loop is bound by the vector ALU, not by LDS.
//                     The (2 my + 1) ceil((2 mx + 1) / 8) lanes of one pass fill 1, 2 or 4 waves; with fewer than four
//                     the waves that are left take other row ranges of the tile (RG_TH / S rows each) and the S partial
//                     sums are added in LDS in ascending order; with more than 256 the tile is taken by several
//                     workgroups (chunks).  Every accumulator is one fmaf chain over i ascending, then j ascending.
// reduce_kernel       the partial surfaces of the tiles of a frame, added in ascending tile order by one thread each.
//                     No atomics: the bits of a frame depend on the frame, t' and the geometry, not on n or the group.
// peak_kernel         64 lanes per frame: lane l scans the entries l, l + 64, ... in row-major order and keeps its first
//                     maximum, lane 0 then takes the first maximum of the 64.  NaN never wins.
// apply_kernel        one thread per output pixel.  A frame whose weights are (1, 0, 0, 0) is copied (converted exactly
//                     or quantised when the element types differ, no arithmetic); every other frame is
//                     (w00 a + w01 b) + (w10 c + w11 d), each operation rounded on its own (contraction is off).
#include "pmd_common.h"
#include "../../include/pmd_hip.h"

namespace {

constexpr int RG_TH = 32;            // window rows of a tile
constexpr int RG_TW = 64;            // window columns of a tile
constexpr int RG_R = 8;              // consecutive sx of a lane
constexpr int RG_THREADS = 256;
constexpr size_t RG_WS_TARGET = 64u << 20;   // tile partials of one launch group, about

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct rg_plan {
  int h, w, nsy, nsx, nq, items, wps, S, chunks, ldw, tiles_x, tiles_y, ntiles;
  size_t lds_bytes, frame_floats;    // partial floats of one frame
};

rg_plan rg_make_plan(int d1, int d2, int my, int mx) {
  rg_plan p;
  p.h = d1 - 2 * my, p.w = d2 - 2 * mx;
  p.nsy = 2 * my + 1, p.nsx = 2 * mx + 1;
  p.nq = (p.nsx + RG_R - 1) / RG_R;
  p.items = p.nsy * p.nq;
  p.wps = p.items <= 64 ? 1 : (p.items <= 128 ? 2 : 4);      // waves of one pass over the items
  p.S = 4 / p.wps;                                           // row ranges of the tile
  p.chunks = (p.items + 64 * p.wps - 1) / (64 * p.wps);      // > 1 only when wps == 4
  p.ldw = RG_R * p.nq + RG_TW + 4;                           // = 4 mod 8; the last window read ends at 8 nq + 63
  p.tiles_x = (p.w + RG_TW - 1) / RG_TW, p.tiles_y = (p.h + RG_TH - 1) / RG_TH;
  p.ntiles = p.tiles_x * p.tiles_y;
  p.lds_bytes = (size_t)(RG_TH + 2 * my) * p.ldw * sizeof(float);
  p.frame_floats = (size_t)p.ntiles * p.nsy * p.nsx;
  return p;
}

template <typename E>
__global__ __launch_bounds__(RG_THREADS) void correlate_kernel(const E* __restrict__ X, long fs, long rs, int my, int mx,
                                                                int h, int w, const float* __restrict__ tp, int tiles_x,
                                                                int ntiles, int nq, int items, int wps, int S, int chunks,
                                                                int ldw, float* __restrict__ P) {
  extern __shared__ float rg_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile = (int)blockIdx.x / chunks, chunk = (int)blockIdx.x % chunks;
  const int i0 = tile / tiles_x * RG_TH, j0 = tile % tiles_x * RG_TW;
  const int th = min(RG_TH, h - i0), tw = min(RG_TW, w - j0);
  const int nsy = 2 * my + 1, nsx = 2 * mx + 1;
  const int lrows = th + 2 * my, lcols = tw + 2 * mx;       // the halo: frame rows i0 .. i0 + lrows, all inside the frame
  const E* F = X + (long)blockIdx.y * fs + (long)i0 * rs + j0;

  for (int r = wave; r < lrows; r += RG_THREADS / 64) {
    const E* row = F + (long)r * rs;
    for (int c = lane; c < ldw; c += 64) rg_lds[r * ldw + c] = c < lcols ? (float)row[c] : 0.f;
  }
  __syncthreads();

  const int split = wave / wps;
  const int item = chunk * 64 * wps + (wave % wps) * 64 + lane;
  const bool active = item < items;
  const int sy = active ? item / nq : 0, q = active ? item % nq : 0;
  const int rows_per = RG_TH / S;
  const int ia = split * rows_per, ib = min(th, ia + rows_per);
  float acc[RG_R];
#pragma unroll
  for (int r = 0; r < RG_R; ++r) acc[r] = 0.f;

  for (int i = ia; i < ib; ++i) {
    const float* __restrict__ trow = tp + (long)(i0 + i) * w + j0;           // the same in every lane of the wave
    const float* frow = rg_lds + (i + sy) * ldw + RG_R * q;
    f32x4 wa = *reinterpret_cast<const f32x4*>(frow), wb = *reinterpret_cast<const f32x4*>(frow + 4);
    int j = 0;
    for (; j + 4 <= tw; j += 4) {
      const f32x4 wc = *reinterpret_cast<const f32x4*>(frow + j + 8);
      const float v[12] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w, wc.x, wc.y, wc.z, wc.w};
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const float t = trow[j + jj];
#pragma unroll
        for (int r = 0; r < RG_R; ++r) acc[r] = __builtin_fmaf(t, v[jj + r], acc[r]);
      }
      wa = wb, wb = wc;
    }
    if (j < tw) {                                                            // the last 1 .. 3 columns of the tile
      const f32x4 wc = *reinterpret_cast<const f32x4*>(frow + j + 8);
      const float v[12] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w, wc.x, wc.y, wc.z, wc.w};
#pragma unroll
      for (int jj = 0; jj < 3; ++jj) {
        if (j + jj < tw) {
          const float t = trow[j + jj];
#pragma unroll
          for (int r = 0; r < RG_R; ++r) acc[r] = __builtin_fmaf(t, v[jj + r], acc[r]);
        }
      }
    }
  }

  if (S > 1) {                         // the row ranges, added in ascending order by the lanes of range 0
    __syncthreads();                   // every wave has finished reading the halo
    const int slot = ((wave % wps) * 64 + lane) * RG_R, per = 64 * wps * RG_R;
    if (split > 0) {
#pragma unroll
      for (int r = 0; r < RG_R; ++r) rg_lds[(split - 1) * per + slot + r] = acc[r];
    }
    __syncthreads();
    if (split == 0) {
      for (int s = 1; s < S; ++s) {
#pragma unroll
        for (int r = 0; r < RG_R; ++r) acc[r] += rg_lds[(s - 1) * per + slot + r];
      }
    }
  }
  if (split == 0 && active) {
    float* out = P + (((long)blockIdx.y * ntiles + tile) * nsy + sy) * nsx + RG_R * q;
#pragma unroll
    for (int r = 0; r < RG_R; ++r)
      if (RG_R * q + r < nsx) out[r] = acc[r];
  }
}

__global__ __launch_bounds__(RG_THREADS) void reduce_kernel(const float* __restrict__ P, int ntiles, int ns,
                                                             float* __restrict__ surf) {
  const int e = (int)blockIdx.x * RG_THREADS + (int)threadIdx.x;
  if (e >= ns) return;
  const float* p = P + (long)blockIdx.y * ntiles * ns + e;
  float s = p[0];
  for (int t = 1; t < ntiles; ++t) s += p[(long)t * ns];
  surf[(long)blockIdx.y * ns + e] = s;
}

__global__ __launch_bounds__(64) void peak_kernel(const float* __restrict__ surf, int my, int mx, int* __restrict__ arg,
                                                  float* __restrict__ peak, float* __restrict__ neigh) {
  __shared__ float bv[64];
  __shared__ int bi[64];
  __shared__ int fin[64];
  const int nsy = 2 * my + 1, nsx = 2 * mx + 1, ns = nsy * nsx;
  const float* s = surf + (long)blockIdx.x * ns;
  const int lane = (int)threadIdx.x;
  float best = 0.f;
  int at = -1, finite = 0;
  for (int e = lane; e < ns; e += 64) {
    const float v = s[e];
    if (v != v) continue;
    finite |= __builtin_isfinite(v) ? 1 : 0;
    if (at < 0 || v > best) best = v, at = e;
  }
  bv[lane] = best, bi[lane] = at, fin[lane] = finite;
  __syncthreads();
  if (lane != 0) return;
  for (int l = 1; l < 64; ++l) {
    finite |= fin[l];
    const int a = bi[l];
    if (a < 0) continue;
    const float v = bv[l];
    if (at < 0 || v > best || (v == best && a < at)) best = v, at = a;
  }
  const float none = __builtin_nanf("");
  float* nb = neigh + (long)blockIdx.x * 9;
  if (at < 0 || !finite) {
    arg[2 * blockIdx.x] = 0, arg[2 * blockIdx.x + 1] = 0;
    peak[blockIdx.x] = none;
    for (int k = 0; k < 9; ++k) nb[k] = none;
    return;
  }
  const int py = at / nsx, px = at % nsx;
  arg[2 * blockIdx.x] = py - my, arg[2 * blockIdx.x + 1] = px - mx;
  peak[blockIdx.x] = best;
  for (int a = -1; a <= 1; ++a)
    for (int b = -1; b <= 1; ++b) {
      const int y = py + a, x = px + b;
      nb[(a + 1) * 3 + (b + 1)] = y >= 0 && y < nsy && x >= 0 && x < nsx ? s[y * nsx + x] : none;
    }
}

template <typename E, typename O>
__global__ __launch_bounds__(RG_THREADS) void apply_kernel(const E* __restrict__ X, long fs, long rs, int d1, int d2,
                                                            const int* __restrict__ ishift, const float* __restrict__ wts,
                                                            int constant, float fill, O* __restrict__ out, long ofs,
                                                            long ors) {
#pragma clang fp contract(off)
  const int x = (int)blockIdx.x * RG_THREADS + (int)threadIdx.x, y = (int)blockIdx.y;
  const long f = blockIdx.z;
  if (x >= d2) return;
  const long ya = (long)y + ishift[2 * f], xa = (long)x + ishift[2 * f + 1], yb = ya + 1, xb = xa + 1;
  const float w00 = wts[4 * f], w01 = wts[4 * f + 1], w10 = wts[4 * f + 2], w11 = wts[4 * f + 3];
  const E* F = X + f * fs;
  O* o = out + f * ofs + (long)y * ors + x;
  const bool copy = w00 == 1.f && w01 == 0.f && w10 == 0.f && w11 == 0.f;
  const bool ina = ya >= 0 && ya < d1, inb = yb >= 0 && yb < d1, inc = xa >= 0 && xa < d2, ind = xb >= 0 && xb < d2;
  const long cya = min(max(ya, 0L), (long)d1 - 1), cyb = min(max(yb, 0L), (long)d1 - 1);
  const long cxa = min(max(xa, 0L), (long)d2 - 1), cxb = min(max(xb, 0L), (long)d2 - 1);
  if (copy) {
    if (constant && !(ina && inc)) {
      *o = pmd_quant<O>(fill);
    } else {
      const E v = F[cya * rs + cxa];
      if constexpr (std::is_same<E, O>::value) *o = v;
      else *o = pmd_quant<O>((float)v);
    }
    return;
  }
  float a = (float)F[cya * rs + cxa], b = (float)F[cya * rs + cxb], c = (float)F[cyb * rs + cxa],
        d = (float)F[cyb * rs + cxb];
  if (constant) {
    if (!(ina && inc)) a = fill;
    if (!(ina && ind)) b = fill;
    if (!(inb && inc)) c = fill;
    if (!(inb && ind)) d = fill;
  }
  const float top = w00 * a + w01 * b, bot = w10 * c + w11 * d;
  *o = pmd_quant<O>(top + bot);
}

template <typename E>
void launch_correlate(pmd_ctx* ctx, const rg_plan& p, const void* X, long fs, long rs, int g, int my, int mx,
                      const float* tp, float* P) {
  const dim3 grid((unsigned)(p.ntiles * p.chunks), (unsigned)g);
  hipLaunchKernelGGL(correlate_kernel<E>, grid, dim3(RG_THREADS), p.lds_bytes, ctx->stream, (const E*)X, fs, rs, my, mx,
                     p.h, p.w, tp, p.tiles_x, p.ntiles, p.nq, p.items, p.wps, p.S, p.chunks, p.ldw, P);
}

template <typename E, typename O>
void launch_apply(pmd_ctx* ctx, const void* X, long fs, long rs, int n0, int g, int d1, int d2, const int* ishift,
                  const float* wts, int constant, float fill, void* out, long ofs, long ors) {
  const dim3 grid((unsigned)((d2 + RG_THREADS - 1) / RG_THREADS), (unsigned)d1, (unsigned)g);
  hipLaunchKernelGGL((apply_kernel<E, O>), grid, dim3(RG_THREADS), 0, ctx->stream, (const E*)X + (long)n0 * fs, fs, rs, d1,
                     d2, ishift + 2 * (long)n0, wts + 4 * (long)n0, constant, fill, (O*)out + (long)n0 * ofs, ofs, ors);
}

bool rg_bad_geometry(int d1, int d2, int my, int mx) {
  return my < 1 || my > PMD_SHIFT_MAX || mx < 1 || mx > PMD_SHIFT_MAX || d1 > PMD_SHIFT_MAX_DIM || d2 > PMD_SHIFT_MAX_DIM ||
         d1 - 2 * my < PMD_SHIFT_MIN_WINDOW || d2 - 2 * mx < PMD_SHIFT_MIN_WINDOW;
}

}  // namespace

extern "C" {

size_t pmd_shift_correlate_workspace_bytes(int n, int d1, int d2, int my, int mx) {
  if (n < 1 || rg_bad_geometry(d1, d2, my, mx)) return 0;
  const rg_plan p = rg_make_plan(d1, d2, my, mx);
  const size_t per = p.frame_floats * sizeof(float);
  size_t g = RG_WS_TARGET / per;
  if (g < 1) g = 1;
  if (g > (size_t)n) g = (size_t)n;
  return g * per;
}

int pmd_shift_correlate(pmd_ctx* ctx, const void* X, int elem, long frame_stride, long row_stride, int y0, int x0, int n,
                        int d1, int d2, int my, int mx, const float* tp, float* surf, void* ws, size_t ws_bytes) {
  CTX_CHECK(ctx);
  const char* what = "pmd_shift_correlate";
  if (n < 0) return pmd_fail(ctx, PMD_ERR_ARG, what, "n is negative");
  if (rg_bad_geometry(d1, d2, my, mx))
    return pmd_fail(ctx, PMD_ERR_ARG, what,
                    "max shifts outside 1 .. 31, a side above 16384, or a window d - 2 m below 8 pixels");
  if (pmd_bad_elem(elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown element type");
  if (y0 < 0 || x0 < 0 || row_stride < (long)x0 + d2 || frame_stride < ((long)y0 + d1 - 1) * row_stride + x0 + d2)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "the image at (y0, x0) does not lie inside a row / a frame of the strides");
  if (!X || !tp || !surf) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if (n == 0) return PMD_OK;
  const rg_plan p = rg_make_plan(d1, d2, my, mx);
  const size_t per = p.frame_floats * sizeof(float);
  if (!ws || ws_bytes < per) return pmd_fail(ctx, PMD_ERR_WORKSPACE, what, "workspace smaller than one frame's tile partials");
  long group = (long)(ws_bytes / per);
  if (group > 32768) group = 32768;
  pmd_prof_scope prof__(ctx, "shift_correlate");
  const size_t esize = pmd_elem_size(elem);
  const int ns = p.nsy * p.nsx;
  for (long f0 = 0; f0 < n; f0 += group) {
    const int g = (int)(n - f0 < group ? n - f0 : group);
    const char* x = (const char*)X + ((size_t)f0 * frame_stride + (size_t)y0 * row_stride + x0) * esize;
    pmd_with_elem(elem, [&](auto e) {
      launch_correlate<typename decltype(e)::type>(ctx, p, x, frame_stride, row_stride, g, my, mx, tp, (float*)ws);
    });
    PMD_LAUNCH_CHECK(ctx, "correlate_kernel");
    hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)((ns + RG_THREADS - 1) / RG_THREADS), (unsigned)g), dim3(RG_THREADS), 0,
                       ctx->stream, (const float*)ws, p.ntiles, ns, surf + f0 * ns);
    PMD_LAUNCH_CHECK(ctx, "reduce_kernel");
  }
  return PMD_OK;
}

int pmd_shift_peak(pmd_ctx* ctx, const float* surf, int n, int my, int mx, int* arg, float* peak, float* neigh) {
  CTX_CHECK(ctx);
  const char* what = "pmd_shift_peak";
  if (n < 0) return pmd_fail(ctx, PMD_ERR_ARG, what, "n is negative");
  if (my < 1 || my > PMD_SHIFT_MAX || mx < 1 || mx > PMD_SHIFT_MAX)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "max shifts outside 1 .. 31");
  if (!surf || !arg || !peak || !neigh) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if (n == 0) return PMD_OK;
  pmd_prof_scope prof__(ctx, "shift_peak");
  hipLaunchKernelGGL(peak_kernel, dim3((unsigned)n), dim3(64), 0, ctx->stream, surf, my, mx, arg, peak, neigh);
  PMD_LAUNCH_CHECK(ctx, "peak_kernel");
  return PMD_OK;
}

int pmd_shift_apply(pmd_ctx* ctx, const void* X, int elem, long frame_stride, long row_stride, int n, int d1, int d2,
                    const int* ishift, const float* wts, int border, float fill, void* out, int out_elem,
                    long out_frame_stride, long out_row_stride) {
  CTX_CHECK(ctx);
  const char* what = "pmd_shift_apply";
  if (n < 0) return pmd_fail(ctx, PMD_ERR_ARG, what, "n is negative");
  if (d1 < 1 || d2 < 1 || d1 > PMD_SHIFT_MAX_DIM || d2 > PMD_SHIFT_MAX_DIM)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "frame sides outside 1 .. 16384");
  if (pmd_bad_elem(elem) || pmd_bad_elem(out_elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown element type");
  if (border != PMD_SHIFT_BORDER_NEAREST && border != PMD_SHIFT_BORDER_CONSTANT)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "border is neither nearest (0) nor constant (1)");
  if (pmd_short_strides(frame_stride, row_stride, d1, d2) ||
      pmd_short_strides(out_frame_stride, out_row_stride, d1, d2))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "a stride is shorter than a row / a frame");
  if (!X || !ishift || !wts || !out) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if (n == 0) return PMD_OK;
  if (pmd_images_overlap(X, elem, frame_stride, row_stride, out, out_elem, out_frame_stride, out_row_stride, n, d1, d2))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "X and out overlap");
  pmd_prof_scope prof__(ctx, "shift_apply");
  const int constant = border == PMD_SHIFT_BORDER_CONSTANT;
  for (int n0 = 0; n0 < n; n0 += 32768) {
    const int g = n - n0 < 32768 ? n - n0 : 32768;
    pmd_with_elem(elem, [&](auto e) {
      pmd_with_elem(out_elem, [&](auto o) {
        launch_apply<typename decltype(e)::type, typename decltype(o)::type>(ctx, X, frame_stride, row_stride, n0, g, d1, d2,
                                                                             ishift, wts, constant, fill, out,
                                                                             out_frame_stride, out_row_stride);
      });
    });
    PMD_LAUNCH_CHECK(ctx, "apply_kernel");
  }
  return PMD_OK;
}

}  // extern "C"
