"""
Rigid motion correction by template matching: the step that makes pixel (y, x) the same piece of tissue in every frame,
which everything after it assumes.

``register_movie(movie, out)`` estimates one shift per frame and writes the corrected movie; ``apply_shifts`` is the
second half on its own (a second channel, shifts from elsewhere); ``RegisteredMovie`` applies the shifts on the host as
frames are requested, so a movie longer than device memory can go into the streamed decomposition without a corrected
copy on disk.  The method is the rigid step of NoRMCorre (Pnevmatikakis & Giovannucci 2017) in its matchTemplate form:

    window   the template's interior, rows [my, d1 - my) x columns [mx, d2 - mx), at least 8 x 8 pixels
    t'       the fp32 template on the window minus its window mean (float64 on the host, rounded once)
    surface  C[dy, dx] = sum over the window of t'[y, x] f[y + dy, x + dx] for |dy| <= my, |dx| <= mx: every term is in
             bounds and every shift sums the same number of terms (scipy.signal.correlate2d(f, t', mode="valid")).
             The un-normalised zero-mean correlation, OpenCV's TM_CCOEFF (pmd_shift_correlate, csrc/register.hip)
    shift    the (dy, dx) that maximises C, the first maximum in row-major order, NaN never wins (pmd_shift_peak); then
             f[y + dy, x + dx] ~ template[y, x] and the corrected frame is out[y, x] = f[y + dy, x + dx]
    finish   a separable three-point parabola on the 3 x 3 neighbourhood of the peak, float64 on the host
             (subpixel_peak)
    apply    integer-shift frames are copied; the others are bilinear, fl(fl(fl(w00 a) + fl(w01 b)) + fl(fl(w10 c) +
             fl(w11 d))) with weights formed in float64 and rounded once (pmd_shift_apply)

The movie is read in the frame batches of the streamed decomposition and handled in blocks of 1024 frames: correlate,
peak, the 48 bytes per frame of the peak tables to the host, the parabola, the weight tables back, apply into the sink.
The shifts of a block are final when its surfaces are (the template is fixed before the pass), so one read serves every
destination.  Device memory does not grow with the movie's length.

``motion_pass`` is that pass, written once for this module and for piecewise.py (which adds a patch estimator and
swaps the applier for its warp); ``register_args`` and ``apply_args`` are the front doors' shared checks.  Destinations,
sinks and the open / finish / abort scaffold under the pass are _sink's.
"""
import functools

import numpy as np

from ._movie import _ELEM, _device_elem, _device_free_bytes, _stream_dtype
from ._sink import HOST_SLOTS, _destination, _optional_destination, check_bigtiff, device_index, movie_pass
from ._stream import BLOCK, _is_int, batch_buffer_bytes, block_plan, check_fit, device_context, each_block
from .dataset import lazy_data_loader
from .spatial import SpatialFilter, as_filter, filter_image, run_filter

MAX_SHIFT = 31               # PMD_SHIFT_MAX
MIN_WINDOW = 8               # PMD_SHIFT_MIN_WINDOW
MAX_DIM = 16384              # PMD_SHIFT_MAX_DIM
MAX_ABS_SHIFT = 1 << 30      # shifts given to apply_shifts: their floors are int32 with room for the + 1
WS_TARGET = 64 << 20         # RG_WS_TARGET of csrc/register.hip: the tile partials of one launch group, about
TILE_ROWS, TILE_COLS = 32, 64
_OUT_DTYPES = ("float32", "uint16", "int16")


# ---- host side: arguments, the template, the parabola, the tables, the host form of the apply step --------------------
def check_max_shift(max_shift, d1, d2):
    """(my, mx) of ``max_shift`` (an int, or a pair) for d1 x d2 frames; each in 1 .. 31, the window at least 8 x 8."""
    if _is_int(max_shift):
        max_shift = (max_shift, max_shift)
    try:
        my, mx = max_shift
    except (TypeError, ValueError):
        raise ValueError("max_shift must be an int or a pair (my, mx), got {!r}".format(max_shift)) from None
    if not _is_int(my) or not _is_int(mx) or not 1 <= my <= MAX_SHIFT or not 1 <= mx <= MAX_SHIFT:
        raise ValueError("max_shift must lie in 1 .. {}, got {!r}".format(MAX_SHIFT, max_shift))
    my, mx = int(my), int(mx)
    if d1 > MAX_DIM or d2 > MAX_DIM:
        raise ValueError("frames of {} x {} are larger than {} pixels a side".format(d1, d2, MAX_DIM))
    if d1 - 2 * my < MIN_WINDOW or d2 - 2 * mx < MIN_WINDOW:
        raise ValueError("max_shift {} leaves a window of {} x {} pixels of the {} x {} frame; it must hold at least "
                         "{} x {}".format((my, mx), d1 - 2 * my, d2 - 2 * mx, d1, d2, MIN_WINDOW, MIN_WINDOW))
    return my, mx


def check_prefilter(prefilter, d1, d2):
    """The SpatialFilter of ``prefilter`` (None, a sigma or a pair of sigmas: a band-pass, or a SpatialFilter) for
    d1 x d2 frames, or None."""
    if prefilter is None:
        return None
    filt = as_filter(prefilter)
    filt.check_frame(d1, d2)
    return filt


def window_template(template, my, mx):
    """t': the fp32 template on the window minus its window mean (taken in float64, rounded once), (h, w) float32."""
    t = np.asarray(template, dtype=np.float32)
    win = t[my:t.shape[0] - my, mx:t.shape[1] - mx]
    mean = np.float32(win.astype(np.float64).mean())
    return np.ascontiguousarray(win - mean, dtype=np.float32)


def _parabola(lo, c, hi):
    lo, c, hi = (np.asarray(v, dtype=np.float64) for v in (lo, c, hi))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        curv = lo - 2.0 * c + hi
        off = 0.5 * (lo - hi) / curv
        ok = np.isfinite(lo) & np.isfinite(c) & np.isfinite(hi) & (curv < 0) & np.isfinite(off)
    return np.where(ok, np.clip(off, -0.5, 0.5), 0.0)


def subpixel_peak(neigh):
    """The sub-pixel offset (..., 2) float64 = (oy, ox) of a peak from its 3 x 3 neighbourhood ``neigh`` (..., 3, 3): a
    three-point parabola per axis through the centre and its two neighbours, (lo - hi) / (2 (lo - 2 c + hi)), clipped to
    [-0.5, 0.5].  An axis's offset is 0 when one of its three values is not finite (a peak on the edge of the search
    range has NaN neighbours there) or when the curvature lo - 2 c + hi is not negative (a flat top)."""
    nb = np.asarray(neigh, dtype=np.float64)
    if nb.shape[-2:] != (3, 3):
        raise ValueError("neigh must end in (3, 3), got shape {}".format(nb.shape))
    return np.stack([_parabola(nb[..., 0, 1], nb[..., 1, 1], nb[..., 2, 1]),
                     _parabola(nb[..., 1, 0], nb[..., 1, 1], nb[..., 1, 2])], axis=-1)


def shift_tables(shifts):
    """(ishift (n, 2) int32, weights (n, 4) float32) of pmd_shift_apply for ``shifts`` (n, 2) float64: the floors and
    the bilinear weights w00, w01, w10, w11 = (1 - fy)(1 - fx), (1 - fy) fx, fy (1 - fx), fy fx, formed in float64 from
    the fractional parts and rounded once."""
    s = np.asarray(shifts, dtype=np.float64).reshape(-1, 2)
    fl = np.floor(s)
    fy, fx = (s - fl)[:, 0], (s - fl)[:, 1]
    w = np.stack([(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx], axis=1)
    return fl.astype(np.int32), np.ascontiguousarray(w.astype(np.float32))


def check_shifts(shifts, T):
    s = np.asarray(shifts)
    if s.dtype.kind not in "iuf" or s.shape != (T, 2):
        raise ValueError("shifts must be a ({}, 2) array of numbers (dy, dx per frame), got {} {}".format(
            T, s.dtype, s.shape))
    s = s.astype(np.float64)
    if not np.all(np.isfinite(s)) or np.any(np.abs(s) > MAX_ABS_SHIFT):
        raise ValueError("shifts must be finite and at most 2^30 in size")
    return s


def check_border(border):
    """(mode, fill): (0, 0.0) for "nearest", (1, value) for a number."""
    if isinstance(border, str):
        if border != "nearest":
            raise ValueError('border must be "nearest" or a number, got {!r}'.format(border))
        return 0, 0.0
    if isinstance(border, (bool, np.bool_)) or not isinstance(border, (int, float, np.integer, np.floating)):
        raise ValueError('border must be "nearest" or a number, got {!r}'.format(border))
    return 1, float(np.float32(border))


def valid_rect(shifts, d1, d2):
    """(y0, y1, x0, x1): the rows [y0, y1) and columns [x0, x1) that no frame filled from outside the image (every
    sample of every frame lies inside it); an empty range when the shifts leave none."""
    s = np.asarray(shifts, dtype=np.float64).reshape(-1, 2)
    if not len(s):
        return 0, int(d1), 0, int(d2)
    lo, hi = np.floor(s).min(axis=0), np.ceil(s).max(axis=0)
    y0, y1 = int(max(0, -lo[0])), int(min(d1, d1 - hi[0]))
    x0, x1 = int(max(0, -lo[1])), int(min(d2, d2 - hi[1]))
    return y0, max(y0, y1), x0, max(x0, x1)


def _quantize(v, dtype):
    from .export import quantize

    return quantize(v, dtype)


def shift_frames(frames, shifts, border="nearest", dtype=None):
    """pmd_shift_apply on the host, with its bits: ``frames`` (n, d1, d2) float32 / uint16 / int16 shifted by ``shifts``
    (n, 2) into ``dtype`` (None: float32, or the frames' own when every shift is an integer)."""
    f = np.asarray(frames)
    n, d1, d2 = f.shape
    mode, fill = check_border(border)
    ish, wts = shift_tables(shifts)
    whole = np.all(wts == np.array([1, 0, 0, 0], np.float32), axis=1)
    out_dtype = np.dtype(dtype) if dtype is not None else (f.dtype if whole.all() else np.dtype(np.float32))
    out = np.empty((n, d1, d2), out_dtype)
    yy, xx = np.arange(d1, dtype=np.int64), np.arange(d2, dtype=np.int64)
    fill32 = np.float32(fill)
    for k in range(n):
        ya, xa = yy + int(ish[k, 0]), xx + int(ish[k, 1])

        def sample(y, x):
            v = f[k][np.clip(y, 0, d1 - 1)[:, None], np.clip(x, 0, d2 - 1)[None, :]]
            inside = ((y >= 0) & (y < d1))[:, None] & ((x >= 0) & (x < d2))[None, :]
            return v, inside

        if whole[k]:
            v, inside = sample(ya, xa)
            if f.dtype != out_dtype:
                v = _quantize(v.astype(np.float32), out_dtype)
            out[k] = np.where(inside, v, _quantize(fill32, out_dtype)) if mode else v
            continue
        vals = []
        for y, x in ((ya, xa), (ya, xa + 1), (ya + 1, xa), (ya + 1, xa + 1)):
            v, inside = sample(y, x)
            v = v.astype(np.float32)
            vals.append(np.where(inside, v, fill32) if mode else v)
        w = wts[k]
        with np.errstate(invalid="ignore", over="ignore"):
            top = (w[0] * vals[0]).astype(np.float32) + (w[1] * vals[1]).astype(np.float32)
            bot = (w[2] * vals[2]).astype(np.float32) + (w[3] * vals[3]).astype(np.float32)
            out[k] = _quantize((top.astype(np.float32) + bot.astype(np.float32)).astype(np.float32), out_dtype)
    return out


def correlate_workspace_bytes(n, d1, d2, my, mx):
    """pmd_shift_correlate_workspace_bytes on the host: the tile partials of min(n, 64 MB worth of) frames."""
    tiles = -(-(d1 - 2 * my) // TILE_ROWS) * -(-(d2 - 2 * mx) // TILE_COLS)
    per = 4 * tiles * (2 * my + 1) * (2 * mx + 1)
    return max(1, min(int(n), WS_TARGET // per)) * per if int(n) >= 1 else 0     # (the library sizes no frames at 0)


def register_device_bytes(*, d1, d2, nb, esize, host_source, n_batches, my=None, mx=None, n_sample=0, out_esize=0,
                          host_dest=False, surfaces=False, prefilter=False):
    """Device bytes register_movie / apply_shifts hold on d1 x d2 frames read in batches of nb; no term grows with the
    movie's length.  The frame batches (two for a host source of more than one batch), and for the estimate (my, mx
    given) t', the tile partials of one launch group, the surfaces of one 1024-frame block (twice when they leave
    through the host ring) and the peak tables; for the template the n_sample sample frames, raw and shifted; for a
    host destination the output ring of two blocks; the per-frame tables of a block; with a prefilter the fp32
    scratch of one filtered block, the filtered sample and the template's two images."""
    D = d1 * d2
    blk = min(BLOCK, nb)
    need = batch_buffer_bytes(nb, D, esize, host_source, n_batches)
    if my is not None:
        ns = (2 * my + 1) * (2 * mx + 1)
        need += 4 * (d1 - 2 * my) * (d2 - 2 * mx) + correlate_workspace_bytes(max(blk, n_sample), d1, d2, my, mx)
        need += (2 if surfaces else 1) * 4 * ns * max(blk, n_sample) + 48 * max(blk, n_sample)
        need += n_sample * D * (esize + 4) + 2 * 4 * D
        if prefilter:
            need += 4 * blk * D + 4 * n_sample * D + 2 * 4 * D
    if host_dest:
        need += HOST_SLOTS * blk * D * out_esize
    return need + 24 * blk + (1 << 20)


class Registration:
    """Result of register_movie: ``shifts`` (T, 2) float64 (dy, dx per frame: out[y, x] = f[y + dy, x + dx]),
    ``integer_shifts`` (T, 2) int32 (the peaks), ``peak`` (T,) float32 (the surface's value there, NaN for a surface
    without a finite entry), ``template`` (d1, d2) float32, ``max_shift`` (my, mx), ``valid`` (y0, y1, x0, x1), the
    rectangle that no frame filled from outside the image (crop to it before decomposing), ``at_limit``, the frames
    whose peak lies on the edge of the search range (their true shift may be larger: a warning, not an error),
    ``border``, ``surfaces`` (T, 2 my + 1, 2 mx + 1) float32 when asked for, else None, and ``prefilter``, the
    SpatialFilter the frames and the template were matched through, or None (``template`` is the unfiltered image
    either way)."""

    def __init__(self, shifts, integer_shifts, peak, template, max_shift, border="nearest", surfaces=None,
                 prefilter=None):
        self.shifts = np.asarray(shifts, dtype=np.float64).reshape(-1, 2)
        self.integer_shifts = np.asarray(integer_shifts, dtype=np.int32).reshape(-1, 2)
        self.peak = np.asarray(peak, dtype=np.float32).reshape(-1)
        self.template = np.asarray(template, dtype=np.float32)
        self.max_shift = (int(max_shift[0]), int(max_shift[1]))
        self.border, self.surfaces, self.prefilter = border, surfaces, prefilter
        d1, d2 = self.template.shape
        self.valid = valid_rect(self.shifts, d1, d2)
        lim = np.abs(self.integer_shifts) == np.array(self.max_shift, dtype=np.int32)[None, :]
        self.at_limit = np.nonzero(lim.any(axis=1))[0]

    def __repr__(self):
        return "Registration({} frames, max_shift {}, {} at the limit, valid {})".format(
            len(self.shifts), self.max_shift, len(self.at_limit), self.valid)


class RegisteredMovie(lazy_data_loader):
    """``movie`` with the shifts of ``registration`` (a Registration, or a (T, 2) array) applied on the host as frames
    are requested: integer shifts are slice copies in the movie's own dtype, fractional shifts the fixed fp32 formula
    of pmd_shift_apply in NumPy (shift_frames), so a frame has the bits of register_movie's output.  ``dtype`` as in
    register_movie (None: the movie's own when every shift is an integer, else float32)."""

    def __init__(self, movie, registration, border=None, dtype=None):
        T, d1, d2 = (int(x) for x in movie.shape)
        shifts = registration.shifts if isinstance(registration, Registration) else registration
        self._shifts = check_shifts(shifts, T)
        if border is None:
            border = registration.border if isinstance(registration, Registration) else "nearest"
        check_border(border)
        self._movie, self._border, self._shape = movie, border, (T, d1, d2)
        self._src_dtype = _stream_dtype(movie)
        whole = bool(np.all(self._shifts == np.floor(self._shifts)))
        self._dtype = _resolve_dtype(dtype, self._src_dtype, whole)

    dtype = property(lambda self: self._dtype)
    shape = property(lambda self: self._shape)

    def _compute_at_indices(self, indices):
        T, d1, d2 = self._shape
        idx = np.arange(T)[indices].reshape(-1)
        key = idx.tolist() if isinstance(self._movie, lazy_data_loader) else idx
        frames = np.asarray(self._movie[key]).reshape(len(idx), d1, d2).astype(self._src_dtype, copy=False)
        return shift_frames(frames, self._shifts[idx], self._border, self._dtype)


def _resolve_dtype(dtype, src_dtype, whole):
    if dtype is None:
        return np.dtype(src_dtype) if whole else np.dtype(np.float32)
    try:
        key = np.dtype(dtype).name
    except TypeError:
        key = None
    if key not in _OUT_DTYPES:
        raise ValueError("dtype must be None or one of {}, got {!r}".format(_OUT_DTYPES, dtype))
    return np.dtype(key)


# ---- device side ----------------------------------------------------------------------------------------------------
def _movie_info(movie):
    """(T, d1, d2, on_device, staged dtype) of a source."""
    import torch

    try:
        shape = tuple(int(x) for x in movie.shape)
    except (AttributeError, TypeError):
        raise TypeError("movie must be an array-like of shape (T, d1, d2), got {}".format(type(movie).__name__)) from None
    if len(shape) != 3:
        raise ValueError("movie must have shape (T, d1, d2), got {}".format(shape))
    if isinstance(movie, torch.Tensor) and movie.device.type != "cpu":
        e = _device_elem(movie[:0])
        return shape + (True, next((dt for dt, code in _ELEM.items() if code == e), np.dtype(np.float32)))
    src = movie.detach().numpy() if isinstance(movie, torch.Tensor) else movie
    return shape + (False, _stream_dtype(src))


class _Estimator:
    """t' on the device with the buffers of one block: surfaces, tile partials, peak tables."""

    def __init__(self, ctx, d1, d2, my, mx, cap, surfaces_out=None):
        import torch

        self.ctx, self.d1, self.d2, self.my, self.mx, self.cap = ctx, d1, d2, my, mx, cap
        self.ns = (2 * my + 1) * (2 * mx + 1)
        dev = ctx.device
        self.tp = torch.empty(((d1 - 2 * my) * (d2 - 2 * mx),), dtype=torch.float32, device=dev)
        self.ws_bytes = int(ctx.lib.pmd_shift_correlate_workspace_bytes(cap, d1, d2, my, mx))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.surf = None if surfaces_out is not None else torch.empty(cap * self.ns, dtype=torch.float32, device=dev)
        self.surfaces_out = surfaces_out           # a _stream.ToHost: the surfaces leave through its ring
        self.arg = torch.empty((cap, 2), dtype=torch.int32, device=dev)
        self.tab = torch.empty(cap * 10, dtype=torch.float32, device=dev)       # m peaks, then m 3 x 3 neighbourhoods

    def set_template(self, template):
        import torch

        self.tp.copy_(torch.from_numpy(window_template(template, self.my, self.mx).reshape(-1)))

    def run(self, X, elem, t0, m):
        """The peaks of the m frames at device address X (contiguous d1 x d2 frames): (arg (m, 2) int32, peak (m,)
        float32, neigh (m, 3, 3) float32) on the host.  Synchronises."""
        import ctypes as C
        from ._lib import ptr

        ctx, d1, d2 = self.ctx, self.d1, self.d2
        if self.surfaces_out is not None:
            buf, _ = self.surfaces_out.dst(t0 * self.ns, m * self.ns)
        else:
            buf = self.surf
        ctx.call("pmd_shift_correlate", X, int(elem), d1 * d2, d2, 0, 0, int(m), d1, d2, self.my, self.mx, ptr(self.tp),
                 ptr(buf), ptr(self.ws), self.ws_bytes)
        peak = C.c_void_p(self.tab.data_ptr())
        neigh = C.c_void_p(self.tab.data_ptr() + 4 * int(m))
        ctx.call("pmd_shift_peak", ptr(buf), int(m), self.my, self.mx, ptr(self.arg), peak, neigh)
        if self.surfaces_out is not None:
            self.surfaces_out.done(t0 * self.ns, m * self.ns)
        arg = self.arg[:m].cpu().numpy()
        tab = self.tab[:10 * m].cpu().numpy()              # the rows in use only
        return arg, tab[:m].copy(), tab[m:].reshape(m, 3, 3).copy()


class _Applier:
    """The per-frame tables of one block on the device, and the call."""

    def __init__(self, ctx, d1, d2, cap, border, out_elem):
        import torch

        self.ctx, self.d1, self.d2, self.out_elem = ctx, d1, d2, out_elem
        self.mode, self.fill = check_border(border)
        self.ish = torch.empty((cap, 2), dtype=torch.int32, device=ctx.device)
        self.wts = torch.empty((cap, 4), dtype=torch.float32, device=ctx.device)

    def run(self, X, elem, m, shifts, out, out_elem=None):
        """out (device address, contiguous frames) = the m frames at X shifted by ``shifts`` (m, 2)."""
        import torch
        from ._lib import ptr

        ish, wts = shift_tables(shifts)
        self.ish[:m].copy_(torch.from_numpy(ish))
        self.wts[:m].copy_(torch.from_numpy(wts))
        D = self.d1 * self.d2
        self.ctx.call("pmd_shift_apply", X, int(elem), D, self.d2, int(m), self.d1, self.d2, ptr(self.ish), ptr(self.wts),
                      self.mode, self.fill, out, self.out_elem if out_elem is None else out_elem, D, self.d2)


def _read_sample(movie, idx, d1, d2, np_dtype, on_device, ctx):
    """The frames ``idx`` of the movie as an (n, D) device tensor in the staged dtype: one strided read."""
    import torch

    if isinstance(movie, torch.Tensor):
        at = torch.from_numpy(idx).to(movie.device)
        if movie.element_size() == 2:                       # gather 16-bit frames as int16: the bits are what matters
            s = movie.view(torch.int16)[at].view(movie.dtype).to(ctx.device)
        else:
            s = movie[at].to(ctx.device)
        want = torch.from_numpy(np.zeros(1, np_dtype)).dtype
        if s.dtype != want:                                 # a dtype the kernels do not read: staged as fp32, as read_batches does
            s = s.to(want)
        return s.reshape(len(idx), d1 * d2).contiguous()
    key = idx.tolist() if isinstance(movie, lazy_data_loader) else idx
    a = np.asarray(movie[key]).reshape(len(idx), d1 * d2)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype)).to(ctx.device)


def sample_frames(T, template_frames):
    """The min(T, template_frames) evenly spaced frames the template is built from."""
    n = min(int(T), int(template_frames))
    return np.unique(np.round(np.linspace(0, T - 1, n)).astype(np.int64))


def _build_template(ctx, est, movie, T, d1, d2, np_dtype, on_device, template_frames, template_iters, filt=None):
    """The mean of the sample frames, refined template_iters times: register the sample to the current template with
    integer shifts, apply them (nearest border), average.  Torch does the averaging.  With ``filt`` the sample is
    filtered once and every iteration matches the filtered sample against the filtered current template; the shifts
    are applied to the unfiltered sample, so the template stays an unfiltered image."""
    import ctypes as C
    import torch

    idx = sample_frames(T, template_frames)
    S = _read_sample(movie, idx, d1, d2, np_dtype, on_device, ctx)
    n, elem = len(idx), _ELEM[np_dtype]
    tmpl = S.to(torch.float32).mean(dim=0)
    if template_iters:
        ap = _Applier(ctx, d1, d2, n, "nearest", 0)
        R = torch.empty((n, d1 * d2), dtype=torch.float32, device=ctx.device)
        M, m_elem = S, elem                                 # what is matched
        if filt is not None:
            M, m_elem = torch.empty((n, d1 * d2), dtype=torch.float32, device=ctx.device), 0
            run_filter(ctx, filt, C.c_void_p(S.data_ptr()), elem, n, d1, d2, C.c_void_p(M.data_ptr()))
        for _ in range(template_iters):
            current = tmpl.cpu().numpy().reshape(d1, d2)
            est.set_template(current if filt is None else filter_image(ctx, filt, current))
            arg, _, _ = est.run(C.c_void_p(M.data_ptr()), m_elem, 0, n)
            ap.run(C.c_void_p(S.data_ptr()), elem, n, arg.astype(np.float64), C.c_void_p(R.data_ptr()))
            tmpl = R.mean(dim=0)
    return tmpl.cpu().numpy().reshape(d1, d2)


def _check_counts(template_frames, template_iters):
    if not _is_int(template_frames) or template_frames < 1:
        raise ValueError("template_frames must be an int >= 1, got {!r}".format(template_frames))
    if not _is_int(template_iters) or template_iters < 0:
        raise ValueError("template_iters must be an int >= 0, got {!r}".format(template_iters))


def motion_pass(what, movie, info, dest, out_dtype, frame_batch_size, num_workers, device, ctx, device_bytes, *,
                estimate=None, patches=None, applier=None, given=None, prefilter=None):
    """The one pass of register_movie / apply_shifts and of register_piecewise / apply_field: per 1024-frame block
    estimate the shifts or take them from ``given`` (indexed by frame), and apply them into ``dest`` when there is one
    (_sink.movie_pass).  Returns (what the estimate found, what dest.close() returned).

    ``estimate``: None, or the rigid step's dict(my, mx, template, template_frames, template_iters, subpixel, surfaces);
    the pass builds the template when it is None, brings the surfaces to the host through a ring when asked, and keeps
    the ``found`` tables template, arg, peak, shifts.  ``patches(ctx, cap)``: None, or what refines a block's rigid
    shifts (piecewise._PatchEstimator: set_template, tables, refine).  ``applier(ctx, cap)``: an _Applier or a
    piecewise._Warper, built when there is a destination.  ``device_bytes(**terms)``: the caller's device-memory bound
    on the terms the pass knows, checked before anything is allocated.  ``prefilter``: None, or the SpatialFilter the
    estimate looks through: every block is filtered into an fp32 scratch that the rigid and the patch estimator read,
    the template is filtered with the same kernel, and the applier still reads the unfiltered block."""
    import ctypes as C
    from ._stream import ToHost

    T, d1, d2, on_device, np_dtype = info
    plan = block_plan(T, frame_batch_size)
    nb = plan[0][1] - plan[0][0] if plan else 0
    found = {}
    with device_context(None, device, ctx) as (ctx, _):
        n_sample = 0
        if estimate is not None and estimate["template"] is None:
            n_sample = len(sample_frames(T, estimate["template_frames"]))
        need = device_bytes(d1=d1, d2=d2, nb=nb, esize=np_dtype.itemsize, host_source=not on_device, n_batches=len(plan),
                            n_sample=n_sample, out_esize=out_dtype.itemsize if dest is not None else 0,
                            host_dest=dest is not None and dest.kind != "device")
        check_fit(what, need, _device_free_bytes(ctx.device))
        cap = max(1, min(BLOCK, nb))
        est = pest = ring = scratch = None
        if estimate is not None:
            my, mx, template = estimate["my"], estimate["mx"], estimate["template"]
            if template is None:
                pre = _Estimator(ctx, d1, d2, my, mx, max(1, n_sample))
                template = _build_template(ctx, pre, movie, T, d1, d2, np_dtype, on_device, estimate["template_frames"],
                                           estimate["template_iters"], prefilter)
                del pre
            if estimate["surfaces"]:
                ring = ToHost(ctx, 1, T * (2 * my + 1) * (2 * mx + 1))
            est = _Estimator(ctx, d1, d2, my, mx, cap, ring)
            matched = template                              # what the estimators match: the template as the frames are seen
            if prefilter is not None:
                import torch

                matched = filter_image(ctx, prefilter, template)
                scratch = torch.empty(cap * d1 * d2, dtype=torch.float32, device=ctx.device)
            est.set_template(matched)
            found.update(template=template, arg=np.zeros((T, 2), np.int32), peak=np.zeros(T, np.float32),
                         shifts=np.zeros((T, 2), np.float64))
            if patches is not None:
                pest = patches(ctx, cap)
                pest.set_template(matched)
                found.update(pest.tables(T))
        ap = applier(ctx, cap) if dest is not None else None

        def write(c0, m, yp, elem, out):
            if est is not None:
                seen, seen_elem = yp, elem
                if scratch is not None:
                    seen, seen_elem = C.c_void_p(scratch.data_ptr()), 0
                    run_filter(ctx, prefilter, yp, elem, m, d1, d2, seen)
                arg, peak, neigh = est.run(seen, seen_elem, c0, m)
                sh = arg.astype(np.float64)
                if estimate["subpixel"]:
                    sh = sh + subpixel_peak(neigh)
                sl = slice(c0, c0 + m)
                found["arg"][sl], found["peak"][sl], found["shifts"][sl] = arg, peak, sh
                if pest is not None:
                    # est.arg still holds the integer peaks of this block on the device: they are the centres
                    sh = pest.refine(seen, seen_elem, m, est.arg, arg, sh, estimate["subpixel"], found, sl)
            else:
                sh = given[c0:c0 + m]
            if out is not None:
                ap.run(yp, elem, m, sh, out)

        def blocks(each):
            each_block(ctx, movie, plan, d1 * d2, frame_batch_size, num_workers)(each)
            if ring is not None:
                ring.finish()

        res = movie_pass(ctx, dest, (d1, d2), out_dtype, cap, blocks, write)
        if ring is not None:
            found["surfaces"] = ring.out.reshape(T, 2 * my + 1, 2 * mx + 1)
        return found, res


def _check_no_alias(movie, out):
    """Raise ValueError when the destination shares memory with the movie: frames would be overwritten before they are
    read (a block is shifted out of the batch it was read into, and a device tensor is sliced in place)."""
    import torch

    shared = False
    if isinstance(movie, torch.Tensor) and isinstance(out, torch.Tensor):
        shared = (movie.device == out.device and movie.numel() > 0 and out.numel() > 0 and
                  movie.untyped_storage().data_ptr() == out.untyped_storage().data_ptr())
    elif isinstance(movie, np.ndarray) and isinstance(out, np.ndarray):
        shared = np.may_share_memory(movie, out)
    if shared:
        raise ValueError("out shares memory with the movie; registration is not done in place")


def _check_stream_args(frame_batch_size, bigtiff):
    if not _is_int(frame_batch_size) or frame_batch_size < 1:
        raise ValueError("frame_batch_size must be an int >= 1, got {!r}".format(frame_batch_size))
    check_bigtiff(bigtiff)


def register_args(movie, out, geometry, template, template_frames, template_iters, frame_batch_size, bigtiff, border,
                  out_dtype_of, device, ctx):
    """The argument checks of register_movie and register_piecewise, in their order: (info, geometry(d1, d2), the fp32
    template or None, the output dtype out_dtype_of(the movie's staged dtype), the destination or None)."""
    info = _movie_info(movie)
    T, d1, d2, _, np_dtype = info
    if T < 1:
        raise ValueError("the movie has no frames")
    geo = geometry(d1, d2)
    _check_counts(template_frames, template_iters)
    _check_stream_args(frame_batch_size, bigtiff)
    check_border(border)
    if template is not None:
        template = np.asarray(template)
        if template.dtype.kind not in "iuf" or template.shape != (d1, d2):
            raise ValueError("template must be a ({}, {}) image of numbers, got {} {}".format(d1, d2, template.dtype,
                                                                                               template.shape))
        template = np.ascontiguousarray(template, dtype=np.float32)
    out_dtype = out_dtype_of(np_dtype)
    if out is not None:
        _check_no_alias(movie, out)
    dest = _optional_destination(out, (T, d1, d2), out_dtype, bigtiff, device_index(None, device, ctx))
    return info, geo, template, out_dtype, dest


def apply_args(what, movie, out, given_of, frame_batch_size, bigtiff, border, out_dtype_of, device, ctx):
    """The argument checks of apply_shifts and apply_field, in their order: (info, given_of(T, d1, d2), the output dtype
    out_dtype_of(the movie's staged dtype, given), the destination)."""
    info = _movie_info(movie)
    T, d1, d2, _, np_dtype = info
    if T < 1:
        raise ValueError("the movie has no frames")
    if d1 > MAX_DIM or d2 > MAX_DIM:
        raise ValueError("frames of {} x {} are larger than {} pixels a side".format(d1, d2, MAX_DIM))
    given = given_of(T, d1, d2)
    _check_stream_args(frame_batch_size, bigtiff)
    check_border(border)
    out_dtype = out_dtype_of(np_dtype, given)
    if out is None:
        raise TypeError("{} needs a destination".format(what))
    _check_no_alias(movie, out)
    dest = _destination(out, (T, d1, d2), out_dtype, bigtiff, device_index(None, device, ctx))
    return info, given, out_dtype, dest


def register_movie(movie, out=None, *, max_shift=15, template=None, template_frames=200, template_iters=2,
                   subpixel=True, border="nearest", dtype=None, frame_batch_size=10000, num_workers=0, bigtiff=None,
                   return_surfaces=False, prefilter=None, device=None, ctx=None):
    """Estimate one rigid shift per frame of ``movie`` ((T, d1, d2): NumPy arrays and memmaps, any lazy_data_loader
    (TiffArray included), CPU tensors, device tensors; the sources of export_movie) against a template, and write the
    corrected movie ``out[t, y, x] = movie[t, y + dy_t, x + dx_t]`` to ``out`` (the destinations of export_movie: a
    .tif / .tiff or .npy path, a host array, a contiguous device tensor; None: only estimate).  Returns a Registration.

    ``max_shift`` = (my, mx), or one int for both, each in 1 .. 31; the template's interior that is left, rows
    [my, d1 - my) x columns [mx, d2 - mx), must hold at least 8 x 8 pixels.  The shift of a frame maximises the
    un-normalised zero-mean cross-correlation of that interior with the frame over |dy| <= my, |dx| <= mx (ties: the
    first in row-major order; NaN never wins; a surface without a finite entry gives shift 0 and peak NaN).
    ``subpixel`` adds the offset of a three-point parabola per axis (subpixel_peak).  Frames whose peak lies on the
    edge of the search range are listed in ``at_limit``.

    ``template``: a (d1, d2) image, or None: the mean of min(T, template_frames) evenly spaced frames (one strided
    read), refined ``template_iters`` times by registering those frames to it with integer shifts and averaging.

    ``prefilter``: None, or a spatial filter the shifts are estimated through: a sigma or a pair (sy, sx) (the
    band-pass of spatial_filter), or a SpatialFilter.  Every frame and the template are filtered before they are
    matched and the shifts are applied to the unfiltered frames; one-photon movies, whose smooth background is fixed
    in the sensor frame, need it.  ``template`` is given, built and returned as an unfiltered image, so
    ``template=reg.template, prefilter=reg.prefilter`` reproduces a run.

    ``border``: "nearest" (samples outside the frame are those of the nearest edge pixel) or a number that replaces
    them.  ``dtype``: "float32", "uint16", "int16" (round half to even, saturating, NaN -> 0), or None: the movie's
    own dtype when every shift is an integer (``subpixel=False``), else float32.  Integer-shift frames are copied bit
    for bit; the others are bilinear in fp32, each operation rounded on its own.

    Reads: the template's sample frames once, then every frame of the movie once, whatever the destination: a block's
    shifts are final as soon as its surfaces are, so the block is corrected while it is still on the device.  Every
    output bit is the same for every frame_batch_size, source and destination.  Device memory does not grow with the
    movie's length (register_device_bytes is checked before anything is allocated); ``return_surfaces=True`` brings the
    (T, 2 my + 1, 2 mx + 1) surfaces to the host through a ring.  Argument errors are raised before any device work
    and before a file is created; a file this call created is removed when it fails midway.  ``out`` must not share memory with the movie."""
    info, ((my, mx), filt), template, out_dtype, dest = register_args(
        movie, out, lambda d1, d2: (check_max_shift(max_shift, d1, d2), check_prefilter(prefilter, d1, d2)), template,
        template_frames, template_iters,
        frame_batch_size, bigtiff, border, lambda src: _resolve_dtype(dtype, src, not subpixel), device, ctx)
    _, d1, d2 = info[:3]
    estimate = dict(my=my, mx=mx, template=template, template_frames=int(template_frames),
                    template_iters=int(template_iters), subpixel=bool(subpixel), surfaces=bool(return_surfaces))
    found, _ = motion_pass("register_movie", movie, info, dest, out_dtype, int(frame_batch_size), num_workers, device, ctx,
                           functools.partial(register_device_bytes, my=my, mx=mx, surfaces=bool(return_surfaces),
                                             prefilter=filt is not None),
                           estimate=estimate, prefilter=filt,
                           applier=lambda ctx, cap: _Applier(ctx, d1, d2, cap, border, _ELEM[out_dtype]))
    return Registration(found["shifts"], found["arg"], found["peak"], found["template"], (my, mx), border,
                        found.get("surfaces"), filt)


def apply_shifts(movie, out, shifts, *, border="nearest", dtype=None, frame_batch_size=10000, num_workers=0,
                 bigtiff=None, device=None, ctx=None):
    """The second half of register_movie on its own: write ``movie`` shifted by ``shifts`` ((T, 2) numbers, or a
    Registration) to ``out``, ``out[t, y, x] = movie[t, y + dy_t, x + dx_t]``; for a second channel, or shifts from
    elsewhere (of any size).  Sources, destinations, ``border`` and ``dtype`` are those of register_movie (None: the
    movie's own dtype when every shift is an integer, else float32).  The movie is read once.  Returns the path or the
    array."""
    def given_of(T, d1, d2):
        return check_shifts(shifts.shifts if isinstance(shifts, Registration) else shifts, T)

    info, given, out_dtype, dest = apply_args(
        "apply_shifts", movie, out, given_of, frame_batch_size, bigtiff, border,
        lambda src, sh: _resolve_dtype(dtype, src, bool(np.all(sh == np.floor(sh)))), device, ctx)
    _, d1, d2 = info[:3]
    _, res = motion_pass("apply_shifts", movie, info, dest, out_dtype, int(frame_batch_size), num_workers, device, ctx,
                         register_device_bytes, given=given,
                         applier=lambda ctx, cap: _Applier(ctx, d1, d2, cap, border, _ELEM[out_dtype]))
    return res
