"""
Piecewise-rigid motion correction: the step of NoRMCorre (Pnevmatikakis & Giovannucci 2017) that register_movie leaves
out.  A two-photon field does not move rigidly (raster scanning turns fast motion into shear, tissue deforms), so the
template is cut into overlapping patches, every patch is matched a few pixels around the frame's own rigid shift, and
the frame is warped by the smooth field that the patch shifts span.

``register_piecewise(movie, out)`` estimates the field of every frame and writes the corrected movie; ``apply_field``
is the second half on its own (a second channel); ``WarpedMovie`` applies the field on the host as frames are requested
(the counterpart of RegisteredMovie); ``warp_frames`` is the warp on the host with the kernel's bits.  The arithmetic:

    rigid     register_movie's: the integer peak (cy, cx) and the sub-pixel rigid shift of every frame
    area      rows [oy, d1 - oy) x columns [ox, d2 - ox) of the template, oy = my + ey, ox = mx + ex (max_shift plus
              max_deviation), Hh x Ww pixels: every term of every patch surface is inside the frame
    patches   ph x pw at strides sy <= ph, sx <= pw; row starts a_i = min(i sy, Hh - ph), i < gy = 1 + ceil((Hh - ph) / sy);
              t'_p = the fp32 template on patch p minus the patch's own mean (float64, rounded once)
    surfaces  C[v, u] = sum t'_p[i, j] f[oy + a + i + cy + v - ey, ox + b + j + cx + u - ex], 0 <= v <= 2 ey, 0 <= u <= 2 ex
              (pmd_patch_correlate, csrc/piecewise.hip); their peaks are pmd_shift_peak's with (my, mx) = (ey, ex)
    shift     (cy + dy_p, cx + dx_p) + subpixel_peak(neigh), float64 on the host; a patch without a finite surface entry
              or with t'_p = 0 takes the frame's rigid shift (``fallback``)
    field     bilinear between the patch centres yc_i = oy + a_i + (ph - 1) / 2, constant beyond the outermost ones, in
              fp32 in difference form (field_tables, lerp_field)
    warp      out[y, x] = the frame sampled bilinearly at (y + s_y, x + s_x), in fp32, each operation rounded on its own
              (pmd_warp_apply; warp_frames is the same on the host)

The movie is read once in blocks of 1024 frames: rigid correlate and peak, the peak tables to the host, patch correlate
(in sub-blocks of frames, so that the surfaces stay under SURFACE_CAP) and peak, the patch peak tables to the host, the
parabola and the fallbacks, the grid back, the warp into the sink.  Device memory does not grow with the movie's length.

The pass itself (register.motion_pass) and the front doors' checks (register.register_args, apply_args) are
register.py's, the destinations and sinks _sink's; this module holds what differs: the patch grid, the field, the warp,
the patch estimator and its finish on the host.
"""
import functools

import numpy as np

from ._movie import _ELEM, _stream_dtype
from ._stream import BLOCK
from .dataset import lazy_data_loader
from .register import (Registration, _is_int, _quantize, _resolve_dtype, apply_args, check_border, check_max_shift,
                       check_prefilter, motion_pass, register_args, register_device_bytes, subpixel_peak, valid_rect)

MAX_DEV = 7                  # PMD_PATCH_MAX_DEV
MAX_PATCHES = 4096           # PMD_PATCH_MAX
MAX_GRID = 64                # PMD_WARP_MAX_GRID
MIN_PATCH = 8                # PMD_SHIFT_MIN_WINDOW
WS_TARGET = 64 << 20         # PW_WS_TARGET of csrc/piecewise.hip
SURFACE_CAP = 32 << 20       # bytes of patch surfaces held at a time
TILE_ROWS, TILE_COLS = 32, 64
MAX_ABS_SHIFT = 1 << 20      # field entries given to apply_field: exact in fp32 next to a pixel index


# ---- host side: the geometry, the field, the warp ---------------------------------------------------------------------
def _pair(value, name):
    if _is_int(value):
        value = (value, value)
    try:
        a, b = value
    except (TypeError, ValueError):
        raise ValueError("{} must be an int or a pair, got {!r}".format(name, value)) from None
    if not _is_int(a) or not _is_int(b):
        raise ValueError("{} must be an int or a pair of ints, got {!r}".format(name, value))
    return int(a), int(b)


def patch_starts(H, p, s):
    """The starts a_i = min(i s, H - p), i < 1 + ceil((H - p) / s), of patches of p pixels at stride s in H pixels."""
    g = 1 + -(-(H - p) // s)
    return np.minimum(np.arange(g, dtype=np.int64) * s, H - p).astype(np.int32)


class PatchGrid:
    """The patches of d1 x d2 frames: ``max_shift`` (my, mx), ``max_deviation`` (ey, ex), the offsets oy, ox, the patch
    area Hh x Ww, ``patch`` (ph, pw), ``stride`` (sy, sx), ``starts`` (ystart (gy,), xstart (gx,)) int32 inside the
    area, ``centers`` (yc (gy,), xc (gx,)) float64 in frame coordinates, gy, gx, P."""

    def __init__(self, d1, d2, max_shift, max_deviation, patch, stride):
        my, mx = check_max_shift(max_shift, d1, d2)
        ey, ex = _pair(max_deviation, "max_deviation")
        if not 1 <= ey <= MAX_DEV or not 1 <= ex <= MAX_DEV:
            raise ValueError("max_deviation must lie in 1 .. {}, got {!r}".format(MAX_DEV, max_deviation))
        oy, ox = my + ey, mx + ex
        Hh, Ww = d1 - 2 * oy, d2 - 2 * ox
        ph, pw = _pair(patch, "patch")
        sy, sx = _pair(stride, "stride")
        if Hh < MIN_PATCH or Ww < MIN_PATCH:
            raise ValueError("max_shift {} and max_deviation {} leave a patch area of {} x {} pixels of the {} x {} "
                             "frame; it must hold at least {} x {}".format((my, mx), (ey, ex), Hh, Ww, d1, d2, MIN_PATCH,
                                                                           MIN_PATCH))
        if not MIN_PATCH <= ph <= Hh or not MIN_PATCH <= pw <= Ww:
            raise ValueError("patch {} must lie between {} x {} and the patch area of {} x {} pixels".format(
                (ph, pw), MIN_PATCH, MIN_PATCH, Hh, Ww))
        if not 1 <= sy <= ph or not 1 <= sx <= pw:
            raise ValueError("stride {} must lie in 1 .. patch {} (no gaps between patches)".format((sy, sx), (ph, pw)))
        ys, xs = patch_starts(Hh, ph, sy), patch_starts(Ww, pw, sx)
        if len(ys) > MAX_GRID or len(xs) > MAX_GRID:
            raise ValueError("patch {} at stride {} gives {} x {} patches; at most {} a side".format(
                (ph, pw), (sy, sx), len(ys), len(xs), MAX_GRID))
        self.d1, self.d2, self.max_shift, self.max_deviation = int(d1), int(d2), (my, mx), (ey, ex)
        self.oy, self.ox, self.Hh, self.Ww, self.patch, self.stride = oy, ox, Hh, Ww, (ph, pw), (sy, sx)
        self.starts = (ys, xs)
        self.centers = (oy + ys + (ph - 1) / 2.0, ox + xs + (pw - 1) / 2.0)
        self.gy, self.gx, self.P = len(ys), len(xs), len(ys) * len(xs)


def patch_templates(template, pg):
    """(t' (P, ph, pw) float32, zero (gy, gx) bool): the fp32 template on every patch minus that patch's own mean (float64,
    rounded once), and the patches whose t' is all zero (a constant template patch: nothing to match)."""
    t = np.asarray(template, dtype=np.float32)
    ph, pw = pg.patch
    out = np.empty((pg.P, ph, pw), np.float32)
    for i, a in enumerate(pg.starts[0]):
        for j, b in enumerate(pg.starts[1]):
            win = t[pg.oy + a:pg.oy + a + ph, pg.ox + b:pg.ox + b + pw]
            out[i * pg.gx + j] = win - np.float32(win.astype(np.float64).mean())
    return out, ~out.reshape(pg.gy, pg.gx, -1).any(axis=2)


def field_tables(centers, d):
    """(idx (d,) int32, w (d,) float32) of one axis: for pixel y the lower centre i0 in 0 .. max(g - 2, 0) and the weight
    clip((y - c_i0) / (c_{i0 + 1} - c_i0), 0, 1) of the upper one (float64, rounded once; 0 for a single centre)."""
    c = np.asarray(centers, dtype=np.float64).reshape(-1)
    y = np.arange(d, dtype=np.float64)
    if len(c) < 2:
        return np.zeros(d, np.int32), np.zeros(d, np.float32)
    if np.any(np.diff(c) <= 0):
        raise ValueError("centers must increase")
    i0 = np.clip(np.searchsorted(c, y, side="right") - 1, 0, len(c) - 2)
    w = np.clip((y - c[i0]) / (c[i0 + 1] - c[i0]), 0.0, 1.0)
    return i0.astype(np.int32), w.astype(np.float32)


def make_tables(centers, d1, d2):
    """(row_idx, row_w, col_idx, col_w) of pmd_warp_apply for the patch ``centers`` (yc, xc)."""
    return field_tables(centers[0], d1) + field_tables(centers[1], d2)


def lerp_field(grid, tables):
    """The (d1, d2, 2) fp32 field of one (gy, gx, 2) grid with the kernel's bits: per component top = fl(g00 + fl(ax
    fl(g01 - g00))), bot the same on the next grid row, s = fl(top + fl(ay fl(bot - top))).  Table indices are clamped
    as the kernel clamps them."""
    g = np.asarray(grid, dtype=np.float32)
    gy, gx = g.shape[:2]
    ri, rw, ci, cw = tables
    ia = np.clip(np.asarray(ri, dtype=np.int64), 0, max(gy - 2, 0))
    ja = np.clip(np.asarray(ci, dtype=np.int64), 0, max(gx - 2, 0))
    ib, jb = np.minimum(ia + 1, gy - 1), np.minimum(ja + 1, gx - 1)
    ax = np.asarray(cw, dtype=np.float32)[None, :, None]
    ay = np.asarray(rw, dtype=np.float32)[:, None, None]
    with np.errstate(invalid="ignore", over="ignore"):
        g00, g01 = g[ia[:, None], ja[None, :]], g[ia[:, None], jb[None, :]]
        g10, g11 = g[ib[:, None], ja[None, :]], g[ib[:, None], jb[None, :]]
        top = g00 + ax * (g01 - g00)
        bot = g10 + ax * (g11 - g10)
        return top + ay * (bot - top)


def _coord(base, s, d):
    """fl(base + s) clamped to [-1, d]; a NaN acts as -1."""
    with np.errstate(invalid="ignore", over="ignore"):
        Y = base + s
        return np.where(Y >= -1, np.minimum(Y, np.float32(d)), np.float32(-1)).astype(np.float32)


def warp_frames(frames, grid, tables, border="nearest", dtype=None):
    """pmd_warp_apply on the host, with its bits: ``frames`` (n, d1, d2) float32 / uint16 / int16 warped by the fields of
    ``grid`` (n, gy, gx, 2) (rounded to fp32) into ``dtype`` (None: float32).  out[y, x] = the frame sampled bilinearly
    at (y + s_y, x + s_x); there is no copy path."""
    f = np.asarray(frames)
    n, d1, d2 = f.shape
    g = np.asarray(grid, dtype=np.float32).reshape((n, -1, np.shape(grid)[-2], 2))
    mode, fill = check_border(border)
    fill32 = np.float32(fill)
    out_dtype = np.dtype(np.float32 if dtype is None else dtype)
    out = np.empty((n, d1, d2), out_dtype)
    yy, xx = np.arange(d1, dtype=np.float32)[:, None], np.arange(d2, dtype=np.float32)[None, :]
    one = np.float32(1)
    for k in range(n):
        s = lerp_field(g[k], tables)
        Y, X = _coord(yy, s[..., 0], d1), _coord(xx, s[..., 1], d2)
        fly, flx = np.floor(Y), np.floor(X)
        fy, fx = Y - fly, X - flx
        ya, xa = fly.astype(np.int64), flx.astype(np.int64)
        vals = []
        for y, x in ((ya, xa), (ya, xa + 1), (ya + 1, xa), (ya + 1, xa + 1)):
            v = f[k][np.clip(y, 0, d1 - 1), np.clip(x, 0, d2 - 1)].astype(np.float32)
            if mode:
                v = np.where((y >= 0) & (y < d1) & (x >= 0) & (x < d2), v, fill32)
            vals.append(v)
        with np.errstate(invalid="ignore", over="ignore"):
            ofy, ofx = one - fy, one - fx
            top = (ofy * ofx) * vals[0] + (ofy * fx) * vals[1]
            bot = (fy * ofx) * vals[2] + (fy * fx) * vals[3]
            out[k] = _quantize((top + bot).astype(np.float32), out_dtype)
    return out


def finish_patches(rigid_shifts, centre, parg, ppeak, pneigh, zero, subpixel=True):
    """The host finish of a block of m frames.  ``rigid_shifts`` (m, 2) float64, ``centre`` (m, 2) the integer rigid
    peaks, ``parg`` (m, gy, gx, 2), ``ppeak`` (m, gy, gx), ``pneigh`` (m, gy, gx, 3, 3) the patch peak tables, ``zero``
    (gy, gx) the patches with t' = 0.  Returns (shifts (m, gy, gx, 2) float64, integer_shifts int32, fallback bool):
    (cy + dy_p, cx + dx_p) + subpixel_peak(neigh); a patch whose peak is NaN (no finite entry) or whose t' is zero takes
    the frame's rigid shift, its integer shift the rigid peak."""
    centre = np.asarray(centre, dtype=np.int32)
    ints = centre[:, None, None, :] + np.asarray(parg, dtype=np.int32)
    sh = ints.astype(np.float64)
    if subpixel:
        sh = sh + subpixel_peak(pneigh)
    fallback = np.isnan(np.asarray(ppeak)) | np.asarray(zero, dtype=bool)[None]
    rigid = np.broadcast_to(np.asarray(rigid_shifts, dtype=np.float64)[:, None, None, :], sh.shape)
    sh = np.where(fallback[..., None], rigid, sh)
    ints = np.where(fallback[..., None], np.broadcast_to(centre[:, None, None, :], ints.shape), ints)
    return sh, ints.astype(np.int32), fallback


def patch_workspace_bytes(n, pg):
    """pmd_patch_correlate_workspace_bytes on the host: the tile partials of min(n, 64 MB worth of) frames."""
    ey, ex = pg.max_deviation
    tiles = -(-pg.patch[0] // TILE_ROWS) * -(-pg.patch[1] // TILE_COLS)
    per = 4 * pg.P * tiles * (2 * ey + 1) * (2 * ex + 1)
    return max(1, min(int(n), WS_TARGET // per)) * per if int(n) >= 1 else 0     # (the library sizes no frames at 0)


def surface_frames(m, pg):
    """Frames whose patch surfaces are held at a time: min(m, SURFACE_CAP worth of), at least one."""
    ey, ex = pg.max_deviation
    return max(1, min(int(m), SURFACE_CAP // (4 * pg.P * (2 * ey + 1) * (2 * ex + 1))))


def piecewise_device_bytes(*, d1, d2, nb, esize, host_source, n_batches, gy, gx, pg=None, n_sample=0, out_esize=4,
                           host_dest=False, prefilter=False):
    """Device bytes register_piecewise / apply_field hold on d1 x d2 frames read in batches of nb; no term grows with the
    movie's length.  Those of register_movie (register_device_bytes); for the estimate (pg given) t' of the patches, the tile
    partials of one launch group, the patch surfaces of one sub-block and the patch peak tables of one block; the grid
    of one block and the four field tables; ``prefilter`` adds register_movie's term."""
    blk = min(BLOCK, nb)
    my, mx = pg.max_shift if pg is not None else (None, None)
    need = register_device_bytes(d1=d1, d2=d2, nb=nb, esize=esize, host_source=host_source, n_batches=n_batches, my=my,
                                 mx=mx, n_sample=n_sample, out_esize=out_esize, host_dest=host_dest, prefilter=prefilter)
    if pg is not None:
        ey, ex = pg.max_deviation
        sub = surface_frames(blk, pg)
        need += 4 * pg.P * pg.patch[0] * pg.patch[1] + patch_workspace_bytes(sub, pg)
        need += 4 * sub * pg.P * (2 * ey + 1) * (2 * ex + 1) + 48 * blk * pg.P + 4 * (pg.gy + pg.gx)
    return need + 8 * blk * gy * gx + 8 * (d1 + d2)


class PiecewiseRegistration:
    """Result of register_piecewise: ``rigid`` (the Registration of the rigid step), ``shifts`` (T, gy, gx, 2) float64
    (dy, dx of every patch of every frame), ``integer_shifts`` (T, gy, gx, 2) int32, ``peak`` (T, gy, gx) float32,
    ``fallback`` (T, gy, gx) bool (the patch took the frame's rigid shift), ``at_limit`` (K, 3) the (t, i, j) whose
    peak lies on the edge of the deviation range (a warning, not an error), ``centers`` (yc, xc), ``starts``, ``patch``,
    ``stride``, ``max_shift``, ``max_deviation``, ``template``, ``border``, ``prefilter`` (that of the rigid step) and
    ``valid`` (y0, y1, x0, x1), valid_rect over all patch shifts: the field is a convex combination of them, so no
    sample of a pixel inside it came from outside the image.  ``field(t)`` is the (d1, d2, 2) fp32 field of frame t with
    the kernel's bits."""

    def __init__(self, rigid, shifts, integer_shifts, peak, fallback, pg, template, border="nearest"):
        self.rigid = rigid
        self.shifts = np.asarray(shifts, dtype=np.float64)
        self.integer_shifts = np.asarray(integer_shifts, dtype=np.int32)
        self.peak = np.asarray(peak, dtype=np.float32)
        self.fallback = np.asarray(fallback, dtype=bool)
        self.centers, self.starts, self.patch, self.stride = pg.centers, pg.starts, pg.patch, pg.stride
        self.max_shift, self.max_deviation = pg.max_shift, pg.max_deviation
        self.template, self.border = np.asarray(template, dtype=np.float32), border
        self.prefilter = getattr(rigid, "prefilter", None)
        self.valid = valid_rect(self.shifts, pg.d1, pg.d2)
        dev = self.integer_shifts - rigid.integer_shifts[:, None, None, :]
        lim = (np.abs(dev) == np.array(self.max_deviation, dtype=np.int32)).any(axis=-1) & ~self.fallback
        self.at_limit = np.argwhere(lim)
        self._tables = make_tables(self.centers, pg.d1, pg.d2)

    def field(self, t):
        return lerp_field(self.shifts[t].astype(np.float32), self._tables)

    def __repr__(self):
        return "PiecewiseRegistration({} frames, {} x {} patches of {}, {} fallbacks, {} at the limit, valid {})".format(
            len(self.shifts), self.shifts.shape[1], self.shifts.shape[2], self.patch, int(self.fallback.sum()),
            len(self.at_limit), self.valid)


def _field_args(registration, centers, T, d1, d2):
    """(shifts (T, gy, gx, 2) float64, centers) of a PiecewiseRegistration, or of a bare array with ``centers``."""
    if isinstance(registration, PiecewiseRegistration):
        shifts, centers = registration.shifts, registration.centers if centers is None else centers
    else:
        shifts = np.asarray(registration)
        if centers is None:
            raise ValueError("a bare array of shifts needs centers=(yc, xc), the patch centres")
    if shifts.dtype.kind not in "iuf" or shifts.ndim != 4 or shifts.shape[0] != T or shifts.shape[3] != 2:
        raise ValueError("shifts must be a ({}, gy, gx, 2) array of numbers, got {} {}".format(T, shifts.dtype, shifts.shape))
    shifts = shifts.astype(np.float64)
    gy, gx = shifts.shape[1:3]
    if not 1 <= gy <= MAX_GRID or not 1 <= gx <= MAX_GRID:
        raise ValueError("the grid of shifts must have 1 .. {} entries a side, got {} x {}".format(MAX_GRID, gy, gx))
    if not np.all(np.isfinite(shifts)) or np.any(np.abs(shifts) > MAX_ABS_SHIFT):
        raise ValueError("shifts must be finite and at most 2^20 in size")
    try:
        yc, xc = (np.asarray(c, dtype=np.float64).reshape(-1) for c in centers)
    except (TypeError, ValueError):
        raise ValueError("centers must be a pair (yc, xc) of increasing coordinates") from None
    if len(yc) != gy or len(xc) != gx:
        raise ValueError("centers of {} x {} entries do not match the {} x {} grid of shifts".format(len(yc), len(xc), gy, gx))
    make_tables((yc, xc), d1, d2)                       # raises when they do not increase
    return shifts, (yc, xc)


class WarpedMovie(lazy_data_loader):
    """``movie`` with the fields of ``registration`` (a PiecewiseRegistration, or a (T, gy, gx, 2) array with
    ``centers``) applied on the host as frames are requested (warp_frames: the bits of register_piecewise's output), so a
    movie longer than device memory can go into the streamed decomposition without a corrected copy on disk.
    ``dtype``: None (float32), "float32", "uint16" or "int16"."""

    def __init__(self, movie, registration, border=None, dtype=None, centers=None):
        T, d1, d2 = (int(x) for x in movie.shape)
        self._shifts, cen = _field_args(registration, centers, T, d1, d2)
        if border is None:
            border = registration.border if isinstance(registration, PiecewiseRegistration) else "nearest"
        check_border(border)
        self._movie, self._border, self._shape = movie, border, (T, d1, d2)
        self._tables = make_tables(cen, d1, d2)
        self._src_dtype = _stream_dtype(movie)
        self._dtype = _resolve_dtype("float32" if dtype is None else dtype, self._src_dtype, False)

    dtype = property(lambda self: self._dtype)
    shape = property(lambda self: self._shape)

    def _compute_at_indices(self, indices):
        T, d1, d2 = self._shape
        idx = np.arange(T)[indices].reshape(-1)
        key = idx.tolist() if isinstance(self._movie, lazy_data_loader) else idx
        frames = np.asarray(self._movie[key]).reshape(len(idx), d1, d2).astype(self._src_dtype, copy=False)
        return warp_frames(frames, self._shifts[idx], self._tables, self._border, self._dtype)


# ---- device side ----------------------------------------------------------------------------------------------------
class _PatchEstimator:
    """t' of the patches on the device with the buffers of one block: start tables, the surfaces of one sub-block, the
    tile partials, the patch peak tables."""

    def __init__(self, ctx, pg, cap):
        import torch

        self.ctx, self.pg, self.cap = ctx, pg, cap
        ey, ex = pg.max_deviation
        self.ns = (2 * ey + 1) * (2 * ex + 1)
        self.sub = surface_frames(cap, pg)
        dev = ctx.device
        self.tp = torch.empty(pg.P * pg.patch[0] * pg.patch[1], dtype=torch.float32, device=dev)
        self.ys = torch.from_numpy(pg.starts[0]).to(dev)
        self.xs = torch.from_numpy(pg.starts[1]).to(dev)
        self.ws_bytes = int(ctx.lib.pmd_patch_correlate_workspace_bytes(self.sub, pg.d1, pg.d2, *pg.max_shift, ey, ex,
                                                                        *pg.patch, pg.gy, pg.gx))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.surf = torch.empty(self.sub * pg.P * self.ns, dtype=torch.float32, device=dev)
        self.arg = torch.empty((cap * pg.P, 2), dtype=torch.int32, device=dev)
        self.tab = torch.empty(cap * pg.P * 10, dtype=torch.float32, device=dev)    # m P peaks, then their neighbourhoods
        self.zero = None

    def set_template(self, template):
        import torch

        tp, self.zero = patch_templates(template, self.pg)
        self.tp.copy_(torch.from_numpy(tp.reshape(-1)))

    def run(self, X, elem, m, centre):
        """The patch peaks of the m frames at device address X around ``centre`` (device, (m, 2) int32): (arg (m, gy, gx,
        2) int32, peak (m, gy, gx) float32, neigh (m, gy, gx, 3, 3) float32) on the host.  Synchronises."""
        import ctypes as C
        from ._lib import ptr

        ctx, pg = self.ctx, self.pg
        ey, ex = pg.max_deviation
        P, esize = pg.P, 4 if int(elem) == 0 else 2
        peak0, neigh0 = self.tab.data_ptr(), self.tab.data_ptr() + 4 * m * P
        for f0 in range(0, m, self.sub):
            g = min(self.sub, m - f0)
            ctx.call("pmd_patch_correlate", C.c_void_p(X.value + f0 * pg.d1 * pg.d2 * esize), int(elem), pg.d1 * pg.d2,
                     pg.d2, g, pg.d1, pg.d2, *pg.max_shift, ey, ex, *pg.patch, pg.gy, pg.gx, ptr(self.ys), ptr(self.xs),
                     C.c_void_p(centre.data_ptr() + 8 * f0), ptr(self.tp), ptr(self.surf), ptr(self.ws), self.ws_bytes)
            ctx.call("pmd_shift_peak", ptr(self.surf), g * P, ey, ex, C.c_void_p(self.arg.data_ptr() + 8 * f0 * P),
                     C.c_void_p(peak0 + 4 * f0 * P), C.c_void_p(neigh0 + 36 * f0 * P))
        arg = self.arg[:m * P].cpu().numpy().reshape(m, pg.gy, pg.gx, 2)
        tab = self.tab[:10 * m * P].cpu().numpy()
        return arg, tab[:m * P].reshape(m, pg.gy, pg.gx).copy(), tab[m * P:].reshape(m, pg.gy, pg.gx, 3, 3).copy()

    def tables(self, T):
        """What the pass finds per frame and patch (motion_pass keeps them next to the rigid tables)."""
        g = (T, self.pg.gy, self.pg.gx)
        return dict(patch_shifts=np.zeros(g + (2,), np.float64), ints=np.zeros(g + (2,), np.int32),
                    ppeak=np.zeros(g, np.float32), fallback=np.zeros(g, bool))

    def refine(self, X, elem, m, centre, arg, rigid, subpixel, found, sl):
        """The patch shifts (m, gy, gx, 2) of a block from its rigid peaks (``centre`` on the device, ``arg`` on the
        host) and rigid shifts: run, then the host finish; the block's rows ``sl`` of the tables are filled."""
        parg, ppeak, pneigh = self.run(X, elem, m, centre)
        sh, ints, fb = finish_patches(rigid, arg, parg, ppeak, pneigh, self.zero, subpixel)
        found["patch_shifts"][sl], found["ints"][sl], found["ppeak"][sl], found["fallback"][sl] = sh, ints, ppeak, fb
        return sh


class _Warper:
    """The field tables and the grid of one block on the device, and the call."""

    def __init__(self, ctx, d1, d2, gy, gx, centers, cap, border, out_elem):
        import torch

        self.ctx, self.d1, self.d2, self.gy, self.gx, self.out_elem = ctx, d1, d2, gy, gx, out_elem
        self.mode, self.fill = check_border(border)
        self.tables = [torch.from_numpy(t).to(ctx.device) for t in make_tables(centers, d1, d2)]
        self.grid = torch.empty((cap, gy, gx, 2), dtype=torch.float32, device=ctx.device)

    def run(self, X, elem, m, shifts, out):
        """out (device address, contiguous frames) = the m frames at X warped by the fields of ``shifts`` (m, gy, gx, 2)."""
        import torch
        from ._lib import ptr

        self.grid[:m].copy_(torch.from_numpy(np.ascontiguousarray(shifts, dtype=np.float32)))
        D = self.d1 * self.d2
        ri, rw, ci, cw = self.tables
        self.ctx.call("pmd_warp_apply", X, int(elem), D, self.d2, int(m), self.d1, self.d2, ptr(self.grid), self.gy, self.gx,
                      ptr(ri), ptr(rw), ptr(ci), ptr(cw), self.mode, self.fill, out, self.out_elem, D, self.d2)


def _out_dtype(dtype):
    return _resolve_dtype("float32" if dtype is None else dtype, np.dtype(np.float32), False)


def register_piecewise(movie, out=None, *, max_shift=15, patch=128, stride=96, max_deviation=3, template=None,
                       template_frames=200, template_iters=2, subpixel=True, border="nearest", dtype=None,
                       frame_batch_size=10000, num_workers=0, bigtiff=None, prefilter=None, device=None, ctx=None):
    """Estimate a smooth shift field per frame of ``movie`` (the sources of register_movie) against a template and write
    the corrected movie ``out[t, y, x] = movie[t] sampled at (y + s_y, x + s_x)`` to ``out`` (the destinations of
    register_movie; None: only estimate).  Returns a PiecewiseRegistration.

    ``max_shift`` = (my, mx) bounds the rigid shift as in register_movie; ``max_deviation`` = (ey, ex), each in 1 .. 7,
    bounds what a patch may move relative to its frame's rigid shift.  ``patch`` = (ph, pw) and ``stride`` = (sy, sx)
    (an int sets both) cut the template's patch area, rows [my + ey, d1 - my - ey) x columns [mx + ex, d2 - mx - ex),
    into patches of at least 8 x 8 pixels at strides of at most a patch (the last patch of a row is pulled back to end
    with the area); at most 64 patches a side.  Every patch is matched against the frame around the frame's integer
    rigid peak by the un-normalised zero-mean correlation; ``subpixel`` adds the parabola's offset to the rigid and to
    the patch shifts.  A patch whose surface has no finite entry, or whose template is constant, takes the frame's
    rigid shift (``fallback``); patches whose peak lies on the edge of the deviation range are listed in ``at_limit``.
    The field of a frame is bilinear between the patch centres and constant beyond the outermost ones; the frame is
    sampled bilinearly in fp32, each operation rounded on its own.

    ``template``, ``template_frames``, ``template_iters`` and ``prefilter`` as in register_movie (the refinement is
    rigid; with a prefilter the rigid and the patch surfaces are those of the filtered frames and the filtered
    template, and the warp reads the unfiltered frames).  ``border``:
    "nearest" or a number.  ``dtype``: "float32" (None), "uint16", "int16".

    Reads: the template's sample frames once, then every frame of the movie once.  Every output bit is the same for every
    frame_batch_size, source and destination.  Device memory does not grow with the movie's length
    (piecewise_device_bytes is checked before anything is allocated).  Argument errors are raised before any device work
    and before a file is created; a file this call created is removed when it fails midway.  ``out`` must not share
    memory with the movie."""
    info, (pg, filt), template, out_dtype, dest = register_args(
        movie, out, lambda d1, d2: (PatchGrid(d1, d2, max_shift, max_deviation, patch, stride),
                                    check_prefilter(prefilter, d1, d2)),
        template, template_frames, template_iters, frame_batch_size, bigtiff, border, lambda src: _out_dtype(dtype), device,
        ctx)
    (my, mx), subpixel = pg.max_shift, bool(subpixel)
    estimate = dict(my=my, mx=mx, template=template, template_frames=int(template_frames),
                    template_iters=int(template_iters), subpixel=subpixel, surfaces=False)
    found, _ = motion_pass(
        "register_piecewise", movie, info, dest, out_dtype, int(frame_batch_size), num_workers, device, ctx,
        functools.partial(piecewise_device_bytes, gy=pg.gy, gx=pg.gx, pg=pg, prefilter=filt is not None),
        estimate=estimate, prefilter=filt,
        patches=lambda ctx, cap: _PatchEstimator(ctx, pg, cap),
        applier=lambda ctx, cap: _Warper(ctx, pg.d1, pg.d2, pg.gy, pg.gx, pg.centers, cap, border, _ELEM[out_dtype]))
    rigid = Registration(found["shifts"], found["arg"], found["peak"], found["template"], pg.max_shift, border,
                         prefilter=filt)
    return PiecewiseRegistration(rigid, found["patch_shifts"], found["ints"], found["ppeak"], found["fallback"], pg,
                                 found["template"], border)


def apply_field(movie, out, registration, *, centers=None, border=None, dtype=None, frame_batch_size=10000,
                num_workers=0, bigtiff=None, device=None, ctx=None):
    """The second half of register_piecewise on its own: write ``movie`` warped by the fields of ``registration`` (a
    PiecewiseRegistration, or a (T, gy, gx, 2) array of patch shifts with ``centers`` = (yc, xc), the increasing frame
    coordinates of the grid's rows and columns) to ``out``; for a second channel, or a field from elsewhere.  Sources,
    destinations, ``border`` (None: the registration's, else "nearest") and ``dtype`` are those of register_piecewise.
    The movie is read once.  Returns the path or the array."""
    if border is None:
        border = registration.border if isinstance(registration, PiecewiseRegistration) else "nearest"
    info, (shifts, cen), out_dtype, dest = apply_args(
        "apply_field", movie, out, lambda T, d1, d2: _field_args(registration, centers, T, d1, d2), frame_batch_size,
        bigtiff, border, lambda src, given: _out_dtype(dtype), device, ctx)
    _, d1, d2 = info[:3]
    gy, gx = shifts.shape[1:3]
    _, res = motion_pass(
        "apply_field", movie, info, dest, out_dtype, int(frame_batch_size), num_workers, device, ctx,
        functools.partial(piecewise_device_bytes, gy=gy, gx=gx), given=shifts,
        applier=lambda ctx, cap: _Warper(ctx, d1, d2, gy, gx, cen, cap, border, _ELEM[out_dtype]))
    return res
