// Piecewise-rigid motion correction (localmd_amd/piecewise.py): the correlation surfaces of the template's patches,
// searched a few pixels around every frame's own rigid peak (pmd_patch_correlate), and the warp of a frame by the
// smooth field that the patch shifts span (pmd_warp_apply).  The peaks of the patch surfaces are pmd_shift_peak's.
//
// Geometry.  oy = my + ey, ox = mx + ex; the patch area is rows [oy, d1 - oy) x columns [ox, d2 - ox) of the template,
// Hh x Ww pixels.  Patch p = (pi, pj) starts at (a, b) = (ystart[pi], xstart[pj]) of the area and is ph x pw pixels; t'
// is packed (P, ph, pw).  With (cy, cx) the frame's rigid peak, 0 <= v <= 2 ey, 0 <= u <= 2 ex,
//     C[v, u] = sum_{i < ph, j < pw} t'_p[i, j] f[oy + a + i + cy + v - ey, ox + b + j + cx + u - ex],
// every term inside the frame.
//
// patch_correlate_kernel  a workgroup takes one frame, one patch and one PW_TH x PW_TW tile of the patch.  The
//                     (rows + 2 ey) x (columns + 2 ex) halo of the frame is widened to fp32 into LDS once, the tile of
//                     t' next to it.  The rigid kernel's mapping (a lane per (sy, 8 sx)) would keep 7 lanes of a wave
//                     busy on a 7 x 7 surface, so here a lane owns one v, the whole run of u (R = 8 or 16 accumulators
//                     fed from a sliding register window of R + 4 frame values, one 16-byte LDS read per four columns)
//                     and one residue class c of the tile's rows, i = c, c + K, ..., K = min(32, 256 / (2 ey + 1)):
//                     224 of 256 lanes at ey = 3.  t' differs between the lanes of a wave (its row depends on c), so it
//                     is read from LDS too, one 16-byte read per four columns: two LDS reads feed 4 R FMAs.
//                     Every accumulator is one fmaf chain over the rows of its class ascending, then j ascending; the K
//                     classes are added in ascending order through LDS by one lane per entry.
// patch_reduce_kernel the tiles of a (frame, patch) added in ascending (row-major) order by one thread per entry.
//                     No atomics: the bits of a (frame, patch) surface depend on the frame, t'_p, the centre and the
//                     geometry, not on n, the launch group or the other patches.
// warp_kernel         a workgroup takes 256 columns of WP_ROWS consecutive rows of one frame.  The grid rows those
//                     image rows interpolate between (at most WP_ROWS + 1: the row index grows by at most one per image
//                     row) are staged in LDS once, the column index and weight of a thread's pixel are loaded once for
//                     all its rows, the row index and weight are uniform: per pixel there is the frame's four samples,
//                     four 8-byte LDS reads and one store.
#include "pmd_common.h"
#include "../../include/pmd_hip.h"

namespace {

constexpr int PW_TH = 32;            // patch rows of a tile
constexpr int PW_TW = 64;            // patch columns of a tile
constexpr int PW_THREADS = 256;
constexpr size_t PW_WS_TARGET = 64u << 20;   // tile partials of one launch group, about
constexpr int WP_ROWS = 4;           // image rows of a warp workgroup

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct pw_plan {
  int Hh, Ww, nv, nu, R, K, ldw, tiles_x, tiles_y, ntiles, P;
  size_t halo_floats, lds_bytes, frame_floats;    // partial floats of one frame
};

pw_plan pw_make_plan(int d1, int d2, int my, int mx, int ey, int ex, int ph, int pw, int gy, int gx) {
  pw_plan p;
  p.Hh = d1 - 2 * (my + ey), p.Ww = d2 - 2 * (mx + ex);
  p.nv = 2 * ey + 1, p.nu = 2 * ex + 1;
  p.R = p.nu <= 8 ? 8 : 16;
  p.K = PW_THREADS / p.nv < PW_TH ? PW_THREADS / p.nv : PW_TH;
  p.ldw = PW_TW + p.R + 4;                                   // = 4 mod 8; the last window read ends at R + 63
  p.tiles_x = (pw + PW_TW - 1) / PW_TW, p.tiles_y = (ph + PW_TH - 1) / PW_TH;
  p.ntiles = p.tiles_x * p.tiles_y;
  p.P = gy * gx;
  p.halo_floats = (size_t)(PW_TH + 2 * ey) * p.ldw;
  p.lds_bytes = (p.halo_floats + (size_t)PW_TH * PW_TW + (size_t)p.nv * p.K * p.R) * sizeof(float);
  p.frame_floats = (size_t)p.P * p.ntiles * p.nv * p.nu;
  return p;
}

template <typename E, int R>
__global__ __launch_bounds__(PW_THREADS) void patch_correlate_kernel(
    const E* __restrict__ X, long fs, long rs, int my, int mx, int ey, int ex, int ph, int pw, int gx, int Hh, int Ww,
    const int* __restrict__ ystart, const int* __restrict__ xstart, const int* __restrict__ centre,
    const float* __restrict__ tp, int tiles_x, int ntiles, int K, int halo_floats, float* __restrict__ Pp) {
  extern __shared__ __attribute__((aligned(16))) float pw_lds[];
  constexpr int ldw = PW_TW + R + 4;
  float* halo = pw_lds;
  float* tl = pw_lds + halo_floats;
  float* red = tl + PW_TH * PW_TW;
  const int tid = (int)threadIdx.x;
  const int p = (int)blockIdx.x / ntiles, tile = (int)blockIdx.x % ntiles;
  const int i0 = tile / tiles_x * PW_TH, j0 = tile % tiles_x * PW_TW;
  const int th = min(PW_TH, ph - i0), tw = min(PW_TW, pw - j0);
  const int nv = 2 * ey + 1, nu = 2 * ex + 1;
  // a start outside the patch area and a centre outside the search range are clamped: no table can cause a read
  // outside the frame
  const int a = min(max(ystart[p / gx], 0), Hh - ph), b = min(max(xstart[p % gx], 0), Ww - pw);
  const int cy = min(max(centre[2 * blockIdx.y], -my), my), cx = min(max(centre[2 * blockIdx.y + 1], -mx), mx);
  const int lrows = th + 2 * ey, lcols = tw + 2 * ex;
  // halo row 0, column 0: frame row oy + a + i0 + cy - ey = my + a + i0 + cy >= 0; the last one is at most d1 - 1
  const E* F = X + (long)blockIdx.y * fs + (long)(my + a + i0 + cy) * rs + (mx + b + j0 + cx);

  for (int r = tid >> 6; r < lrows; r += PW_THREADS / 64) {
    const E* row = F + (long)r * rs;
    for (int c = tid & 63; c < ldw; c += 64) halo[r * ldw + c] = c < lcols ? (float)row[c] : 0.f;
  }
  const float* T = tp + ((long)p * ph + i0) * pw + j0;
  for (int e = tid; e < PW_TH * PW_TW; e += PW_THREADS) {
    const int i = e / PW_TW, j = e % PW_TW;
    tl[e] = i < th && j < tw ? T[(long)i * pw + j] : 0.f;
  }
  __syncthreads();

  const bool active = tid < nv * K;
  const int c = tid / nv, v = tid % nv;
  float acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.f;

  if (active) {
    for (int i = c; i < th; i += K) {
      const float* trow = tl + i * PW_TW;
      const float* frow = halo + (i + v) * ldw;
      float win[R + 4];
#pragma unroll
      for (int k = 0; k < R; k += 4) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(frow + k);
        win[k] = w.x, win[k + 1] = w.y, win[k + 2] = w.z, win[k + 3] = w.w;
      }
      int j = 0;
      for (; j + 4 <= tw; j += 4) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(frow + j + R);
        win[R] = w.x, win[R + 1] = w.y, win[R + 2] = w.z, win[R + 3] = w.w;
        const f32x4 t4 = *reinterpret_cast<const f32x4*>(trow + j);
        const float t[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
          for (int r = 0; r < R; ++r) acc[r] = __builtin_fmaf(t[jj], win[jj + r], acc[r]);
        }
#pragma unroll
        for (int k = 0; k < R; ++k) win[k] = win[k + 4];
      }
      if (j < tw) {                                                          // the last 1 .. 3 columns of the tile
        const f32x4 w = *reinterpret_cast<const f32x4*>(frow + j + R);
        win[R] = w.x, win[R + 1] = w.y, win[R + 2] = w.z, win[R + 3] = w.w;
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) {
          if (j + jj < tw) {
            const float t = trow[j + jj];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = __builtin_fmaf(t, win[jj + r], acc[r]);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) red[tid * R + r] = acc[r];                   // tid = c nv + v
  }
  __syncthreads();
  if (tid < nv * nu) {                 // the row classes, added in ascending order by one lane per entry
    const int ov = tid / nu, ou = tid % nu;
    float s = red[ov * R + ou];
    for (int k = 1; k < K; ++k) s += red[(k * nv + ov) * R + ou];
    Pp[(((long)blockIdx.y * gridDim.x) + blockIdx.x) * (nv * nu) + tid] = s;
  }
}

__global__ __launch_bounds__(PW_THREADS) void patch_reduce_kernel(const float* __restrict__ Pp, int ntiles, int ns,
                                                                   long total, float* __restrict__ surf) {
  const long e = (long)blockIdx.x * PW_THREADS + threadIdx.x;
  if (e >= total) return;
  const float* p = Pp + (e / ns) * ntiles * ns + e % ns;
  float s = p[0];
  for (int t = 1; t < ntiles; ++t) s += p[(long)t * ns];
  surf[e] = s;
}

// a coordinate: clamped to [-1, d], NaN -> -1, so that its floor is an int in [-1, d] whatever the field holds
__device__ __forceinline__ float pw_coord(float base, float s, int d) {
#pragma clang fp contract(off)
  const float Y = base + s;
  return Y >= -1.f ? fminf(Y, (float)d) : -1.f;
}

template <typename E, typename O>
__global__ __launch_bounds__(PW_THREADS) void warp_kernel(const E* __restrict__ X, long fs, long rs, int d1, int d2,
                                                           const float* __restrict__ grid, int gy, int gx,
                                                           const int* __restrict__ row_idx, const float* __restrict__ row_w,
                                                           const int* __restrict__ col_idx, const float* __restrict__ col_w,
                                                           int constant, float fill, O* __restrict__ out, long ofs,
                                                           long ors) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float g[(WP_ROWS + 1) * PMD_WARP_MAX_GRID * 2];
  const int x = (int)blockIdx.x * PW_THREADS + (int)threadIdx.x, y0 = (int)blockIdx.y * WP_ROWS;
  const long f = blockIdx.z;
  const int ilim = max(gy - 2, 0), jlim = max(gx - 2, 0);
  const int ibase = min(max(row_idx[y0], 0), ilim);            // the first grid row this workgroup needs
  const float* G = grid + f * gy * gx * 2;
  for (int e = (int)threadIdx.x; e < (WP_ROWS + 1) * gx * 2; e += PW_THREADS) {
    const int i = min(ibase + e / (gx * 2), gy - 1);
    g[e] = G[(long)i * gx * 2 + e % (gx * 2)];
  }
  __syncthreads();
  if (x >= d2) return;
  const int ja = min(max(col_idx[x], 0), jlim), jb = min(ja + 1, gx - 1);
  const float ax = col_w[x];
  const E* F = X + f * fs;
  const int yend = min(y0 + WP_ROWS, d1);
  for (int y = y0; y < yend; ++y) {
    const int it = min(max(row_idx[y], 0), ilim), rel = it - ibase;           // uniform over the workgroup
    const float ay = row_w[y];
    // a row table that is not the host layer's (not monotone, or steps above one) may leave the staged rows: those
    // rows read the grid itself
    const int itb = min(it + 1, gy - 1);
    f32x2 g00, g01, g10, g11;
    if (rel >= 0 && rel < WP_ROWS) {
      const float *ga = g + rel * gx * 2, *gb = g + (itb - ibase) * gx * 2;
      g00 = *reinterpret_cast<const f32x2*>(ga + ja * 2), g01 = *reinterpret_cast<const f32x2*>(ga + jb * 2);
      g10 = *reinterpret_cast<const f32x2*>(gb + ja * 2), g11 = *reinterpret_cast<const f32x2*>(gb + jb * 2);
    } else {
      const float *ga = G + (long)it * gx * 2, *gb = G + (long)itb * gx * 2;
      g00 = f32x2{ga[ja * 2], ga[ja * 2 + 1]}, g01 = f32x2{ga[jb * 2], ga[jb * 2 + 1]};
      g10 = f32x2{gb[ja * 2], gb[ja * 2 + 1]}, g11 = f32x2{gb[jb * 2], gb[jb * 2 + 1]};
    }
    const float ty = g00.x + ax * (g01.x - g00.x), by = g10.x + ax * (g11.x - g10.x);
    const float tx = g00.y + ax * (g01.y - g00.y), bx = g10.y + ax * (g11.y - g10.y);
    const float sy = ty + ay * (by - ty), sx = tx + ay * (bx - tx);
    const float Y = pw_coord((float)y, sy, d1), Xc = pw_coord((float)x, sx, d2);
    const float fly = floorf(Y), flx = floorf(Xc);
    const float fy = Y - fly, fx = Xc - flx;
    const int ya = (int)fly, xa = (int)flx, yb = ya + 1, xb = xa + 1;
    const bool ina = ya >= 0 && ya < d1, inb = yb < d1, inc = xa >= 0 && xa < d2, ind = xb < d2;
    const long cya = min(max(ya, 0), d1 - 1), cyb = min(yb, d1 - 1);
    const long cxa = min(max(xa, 0), d2 - 1), cxb = min(xb, d2 - 1);
    float a = (float)F[cya * rs + cxa], b = (float)F[cya * rs + cxb], c = (float)F[cyb * rs + cxa],
          d = (float)F[cyb * rs + cxb];
    if (constant) {
      if (!(ina && inc)) a = fill;
      if (!(ina && ind)) b = fill;
      if (!(inb && inc)) c = fill;
      if (!(inb && ind)) d = fill;
    }
    const float ofy = 1.f - fy, ofx = 1.f - fx;
    const float w00 = ofy * ofx, w01 = ofy * fx, w10 = fy * ofx, w11 = fy * fx;
    const float top = w00 * a + w01 * b, bot = w10 * c + w11 * d;
    out[f * ofs + (long)y * ors + x] = pmd_quant<O>(top + bot);
  }
}

template <typename E>
void launch_patch(pmd_ctx* ctx, const pw_plan& p, const void* X, long fs, long rs, int g, int my, int mx, int ey, int ex,
                  int ph, int pw, int gx, const int* ystart, const int* xstart, const int* centre, const float* tp,
                  float* Pp) {
  const dim3 grid((unsigned)(p.P * p.ntiles), (unsigned)g);
  if (p.R == 8)
    hipLaunchKernelGGL((patch_correlate_kernel<E, 8>), grid, dim3(PW_THREADS), p.lds_bytes, ctx->stream, (const E*)X, fs, rs,
                       my, mx, ey, ex, ph, pw, gx, p.Hh, p.Ww, ystart, xstart, centre, tp, p.tiles_x, p.ntiles, p.K,
                       (int)p.halo_floats, Pp);
  else
    hipLaunchKernelGGL((patch_correlate_kernel<E, 16>), grid, dim3(PW_THREADS), p.lds_bytes, ctx->stream, (const E*)X, fs,
                       rs, my, mx, ey, ex, ph, pw, gx, p.Hh, p.Ww, ystart, xstart, centre, tp, p.tiles_x, p.ntiles, p.K,
                       (int)p.halo_floats, Pp);
}

struct warp_args {
  long fs, rs, ofs, ors;
  int d1, d2, gy, gx, constant;
  float fill;
  const float* grid;
  const int *row_idx, *col_idx;
  const float *row_w, *col_w;
};

template <typename E, typename O>
void launch_warp(pmd_ctx* ctx, const warp_args& a, const void* X, void* out, int n0, int g) {
  const dim3 grid((unsigned)((a.d2 + PW_THREADS - 1) / PW_THREADS), (unsigned)((a.d1 + WP_ROWS - 1) / WP_ROWS), (unsigned)g);
  hipLaunchKernelGGL((warp_kernel<E, O>), grid, dim3(PW_THREADS), 0, ctx->stream, (const E*)X + (long)n0 * a.fs, a.fs, a.rs,
                     a.d1, a.d2, a.grid + (long)n0 * a.gy * a.gx * 2, a.gy, a.gx, a.row_idx, a.row_w, a.col_idx, a.col_w,
                     a.constant, a.fill, (O*)out + (long)n0 * a.ofs, a.ofs, a.ors);
}

bool pw_bad_geometry(int d1, int d2, int my, int mx, int ey, int ex, int ph, int pw, int gy, int gx) {
  if (my < 1 || my > PMD_SHIFT_MAX || mx < 1 || mx > PMD_SHIFT_MAX || ey < 1 || ey > PMD_PATCH_MAX_DEV || ex < 1 ||
      ex > PMD_PATCH_MAX_DEV || d1 < 1 || d2 < 1 || d1 > PMD_SHIFT_MAX_DIM || d2 > PMD_SHIFT_MAX_DIM)
    return true;
  const int Hh = d1 - 2 * (my + ey), Ww = d2 - 2 * (mx + ex);
  return ph < PMD_SHIFT_MIN_WINDOW || pw < PMD_SHIFT_MIN_WINDOW || ph > Hh || pw > Ww || gy < 1 || gx < 1 ||
         gy > PMD_PATCH_MAX || gx > PMD_PATCH_MAX || (long)gy * gx > PMD_PATCH_MAX;
}

}  // namespace

extern "C" {

size_t pmd_patch_correlate_workspace_bytes(int n, int d1, int d2, int my, int mx, int ey, int ex, int ph, int pw, int gy,
                                           int gx) {
  if (n < 1 || pw_bad_geometry(d1, d2, my, mx, ey, ex, ph, pw, gy, gx)) return 0;
  const pw_plan p = pw_make_plan(d1, d2, my, mx, ey, ex, ph, pw, gy, gx);
  const size_t per = p.frame_floats * sizeof(float);
  size_t g = PW_WS_TARGET / per;
  if (g < 1) g = 1;
  if (g > (size_t)n) g = (size_t)n;
  return g * per;
}

int pmd_patch_correlate(pmd_ctx* ctx, const void* X, int elem, long frame_stride, long row_stride, int n, int d1, int d2,
                        int my, int mx, int ey, int ex, int ph, int pw, int gy, int gx, const int* ystart,
                        const int* xstart, const int* centre, const float* tp, float* surf, void* ws, size_t ws_bytes) {
  CTX_CHECK(ctx);
  const char* what = "pmd_patch_correlate";
  if (n < 0) return pmd_fail(ctx, PMD_ERR_ARG, what, "n is negative");
  if (pw_bad_geometry(d1, d2, my, mx, ey, ex, ph, pw, gy, gx))
    return pmd_fail(ctx, PMD_ERR_ARG, what,
                    "max shifts outside 1 .. 31, deviations outside 1 .. 7, a side above 16384, a patch side below 8 or "
                    "above the patch area d - 2 (m + e), or a grid outside 1 .. 4096 patches");
  if (pmd_bad_elem(elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown element type");
  if (pmd_short_strides(frame_stride, row_stride, d1, d2))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "a stride is shorter than a row / a frame");
  if (!X || !ystart || !xstart || !centre || !tp || !surf) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if (n == 0) return PMD_OK;
  const pw_plan p = pw_make_plan(d1, d2, my, mx, ey, ex, ph, pw, gy, gx);
  const size_t per = p.frame_floats * sizeof(float);
  if (!ws || ws_bytes < per) return pmd_fail(ctx, PMD_ERR_WORKSPACE, what, "workspace smaller than one frame's tile partials");
  long group = (long)(ws_bytes / per);
  if (group > 32768) group = 32768;
  pmd_prof_scope prof__(ctx, "patch_correlate");
  const size_t esize = pmd_elem_size(elem);
  const int ns = p.nv * p.nu;
  for (long f0 = 0; f0 < n; f0 += group) {
    const int g = (int)(n - f0 < group ? n - f0 : group);
    const char* x = (const char*)X + (size_t)f0 * frame_stride * esize;
    const int* cen = centre + 2 * f0;
    pmd_with_elem(elem, [&](auto e) {
      launch_patch<typename decltype(e)::type>(ctx, p, x, frame_stride, row_stride, g, my, mx, ey, ex, ph, pw, gx, ystart,
                                               xstart, cen, tp, (float*)ws);
    });
    PMD_LAUNCH_CHECK(ctx, "patch_correlate_kernel");
    const long total = (long)g * p.P * ns;
    hipLaunchKernelGGL(patch_reduce_kernel, dim3((unsigned)((total + PW_THREADS - 1) / PW_THREADS)), dim3(PW_THREADS), 0,
                       ctx->stream, (const float*)ws, p.ntiles, ns, total, surf + f0 * p.P * ns);
    PMD_LAUNCH_CHECK(ctx, "patch_reduce_kernel");
  }
  return PMD_OK;
}

int pmd_warp_apply(pmd_ctx* ctx, const void* X, int elem, long frame_stride, long row_stride, int n, int d1, int d2,
                   const float* grid, int gy, int gx, const int* row_idx, const float* row_w, const int* col_idx,
                   const float* col_w, int border, float fill, void* out, int out_elem, long out_frame_stride,
                   long out_row_stride) {
  CTX_CHECK(ctx);
  const char* what = "pmd_warp_apply";
  if (n < 0) return pmd_fail(ctx, PMD_ERR_ARG, what, "n is negative");
  if (d1 < 1 || d2 < 1 || d1 > PMD_SHIFT_MAX_DIM || d2 > PMD_SHIFT_MAX_DIM)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "frame sides outside 1 .. 16384");
  if (gy < 1 || gy > PMD_WARP_MAX_GRID || gx < 1 || gx > PMD_WARP_MAX_GRID)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "grid sides outside 1 .. 64");
  if (pmd_bad_elem(elem) || pmd_bad_elem(out_elem)) return pmd_fail(ctx, PMD_ERR_ARG, what, "unknown element type");
  if (border != PMD_SHIFT_BORDER_NEAREST && border != PMD_SHIFT_BORDER_CONSTANT)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "border is neither nearest (0) nor constant (1)");
  if (pmd_short_strides(frame_stride, row_stride, d1, d2) ||
      pmd_short_strides(out_frame_stride, out_row_stride, d1, d2))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "a stride is shorter than a row / a frame");
  if (!X || !grid || !row_idx || !row_w || !col_idx || !col_w || !out)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if (n == 0) return PMD_OK;
  if (pmd_images_overlap(X, elem, frame_stride, row_stride, out, out_elem, out_frame_stride, out_row_stride, n, d1, d2))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "X and out overlap");
  pmd_prof_scope prof__(ctx, "warp_apply");
  const warp_args a = {frame_stride, row_stride, out_frame_stride, out_row_stride, d1, d2, gy, gx,
                       border == PMD_SHIFT_BORDER_CONSTANT, fill, grid, row_idx, col_idx, row_w, col_w};
  for (int n0 = 0; n0 < n; n0 += 32768) {
    const int g = n - n0 < 32768 ? n - n0 : 32768;
    pmd_with_elem(elem, [&](auto e) {
      pmd_with_elem(out_elem, [&](auto o) {
        launch_warp<typename decltype(e)::type, typename decltype(o)::type>(ctx, a, X, out, n0, g);
      });
    });
    PMD_LAUNCH_CHECK(ctx, "warp_kernel");
  }
  return PMD_OK;
}

}  // extern "C"
