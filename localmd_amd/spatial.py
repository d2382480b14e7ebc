"""
Separable spatial filtering of a movie's frames: the high-pass that one-photon and miniscope movies need before template
matching (their large smooth background is fixed in the sensor frame, and an un-normalised correlation follows it instead
of the cells), and the band-passed movie that one-photon correlation and PNR images start from.

``spatial_filter(sigma, kind)`` describes a filter, ``filter_frames`` runs it on the host, ``filter_movie`` on the device
over a whole movie; ``register_movie(..., prefilter=)`` and ``register_piecewise(..., prefilter=)`` estimate their shifts
on filtered frames and apply them to the unfiltered ones (NoRMCorre / CaImAN's gSig_filt).

    a(y, x)  float(f[refl(y)][refl(x)]), refl(i) = -1 - i below 0 and 2 d - 1 - i from d on (SciPy's mode="reflect")
    rows     h[y][x] = the chain acc = fl(wx[0] a_0), acc = fl(acc + fl(wx[j] a_j)), a_j = a(y, x + j - rx), j ascending;
             s[y][x] = the chain of fp32 adds of the same a_j
    columns  G = the same chain with wy over h[refl(y + i - ry)][x], S the add chain over s
    out      quant(fl(fl(fl(centre a(y, x)) + G) - fl(box S))); no centre term when centre == 0, no box term when box == 0

    lowpass   centre 0, w = g, box 0                             the Gaussian
    bandpass  centre 0, w = g, box = fp32(1 / ((2 ry + 1)(2 rx + 1)))   the Gaussian minus the window mean, the shape of
                                                                 CaImAN's high_pass_filter_space in separable form
    highpass  centre 1, wy = -gy, wx = gx, box 0                 the frame minus its Gaussian

with g[i] = exp(-(i - r)^2 / 2 sigma^2) normalised to sum 1 in float64 and rounded once to fp32 (pmd_spatial_filter,
csrc/spatial.hip).  Every operation is rounded on its own, so the NumPy float32 form here has the kernel's bits.
"""
import ctypes as C
import math

import numpy as np

from ._movie import _ELEM, _device_free_bytes
from ._sink import HOST_SLOTS, _destination, check_bigtiff, device_index, movie_pass
from ._stream import BLOCK, _is_int, batch_buffer_bytes, block_plan, check_fit, device_context, each_block

MAX_RADIUS = 32              # PMD_FILTER_MAX_RADIUS
MAX_DIM = 16384              # PMD_SHIFT_MAX_DIM
KINDS = ("lowpass", "bandpass", "highpass")
_OUT_DTYPES = ("float32", "uint16", "int16")


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def _pair(value, ok, what):
    if ok(value):
        return value, value
    try:
        a, b = value
    except (TypeError, ValueError):
        a = b = None
    if not ok(a) or not ok(b):
        raise ValueError("{} must be one number or a pair (y, x), got {!r}".format(what, value))
    return a, b


def gaussian_weights(sigma, radius):
    """g[i] = exp(-(i - r)^2 / 2 sigma^2) for i in 0 .. 2 r, normalised to sum 1 in float64, rounded once to fp32."""
    i = np.arange(-radius, radius + 1, dtype=np.float64)
    g = np.exp(-(i * i) / (2.0 * float(sigma) ** 2))
    return np.ascontiguousarray((g / g.sum()).astype(np.float32))


class SpatialFilter:
    """A separable filter of pmd_spatial_filter: ``wy`` (2 ry + 1,) and ``wx`` (2 rx + 1,) float32, ``centre`` and ``box``
    (float), ``ry``, ``rx``; ``sigma`` (sy, sx) and ``kind`` say where the weights came from (None for weights given
    directly)."""

    def __init__(self, wy, wx, centre=0.0, box=0.0, sigma=None, kind=None):
        wy = np.ascontiguousarray(np.asarray(wy, dtype=np.float32).reshape(-1))
        wx = np.ascontiguousarray(np.asarray(wx, dtype=np.float32).reshape(-1))
        for w in (wy, wx):
            if len(w) % 2 != 1 or len(w) > 2 * MAX_RADIUS + 1:
                raise ValueError("a weight array holds 2 r + 1 values with r in 0 .. {}, got {}".format(MAX_RADIUS, len(w)))
        self.wy, self.wx = wy, wx
        self.ry, self.rx = len(wy) // 2, len(wx) // 2
        self.centre, self.box = float(np.float32(centre)), float(np.float32(box))
        self.sigma, self.kind = sigma, kind

    def check_frame(self, d1, d2):
        if not 1 <= d1 <= MAX_DIM or not 1 <= d2 <= MAX_DIM:
            raise ValueError("frames of {} x {} are outside 1 .. {} pixels a side".format(d1, d2, MAX_DIM))
        if self.ry > d1 or self.rx > d2:
            raise ValueError("the filter's radii {} are larger than the {} x {} frame".format((self.ry, self.rx), d1, d2))

    def __repr__(self):
        return "SpatialFilter({}, sigma {}, radius {}, centre {}, box {})".format(
            self.kind, self.sigma, (self.ry, self.rx), self.centre, self.box)


def spatial_filter(sigma, kind="bandpass", radius=None):
    """The SpatialFilter of a Gaussian of ``sigma`` (one positive float, or a pair (sy, sx)) of ``kind`` "lowpass",
    "bandpass" (the Gaussian minus the mean of its (2 ry + 1) x (2 rx + 1) window) or "highpass" (the frame minus its
    Gaussian); ``radius`` (an int or a pair) defaults to ceil(2 sigma) per axis and is at most 32."""
    sy, sx = _pair(sigma, lambda v: _is_number(v) and math.isfinite(v) and v > 0, "sigma (positive)")
    sy, sx = float(sy), float(sx)
    if kind not in KINDS:
        raise ValueError("kind must be one of {}, got {!r}".format(KINDS, kind))
    if radius is None:
        radius = (int(math.ceil(2 * sy)), int(math.ceil(2 * sx)))
    ry, rx = _pair(radius, lambda v: _is_int(v) and v >= 0, "radius (an int >= 0)")
    if ry > MAX_RADIUS or rx > MAX_RADIUS:
        raise ValueError("the radius {} is larger than {}; give a smaller radius".format((int(ry), int(rx)), MAX_RADIUS))
    gy, gx = gaussian_weights(sy, int(ry)), gaussian_weights(sx, int(rx))
    if kind == "lowpass":
        return SpatialFilter(gy, gx, 0.0, 0.0, (sy, sx), kind)
    if kind == "bandpass":
        return SpatialFilter(gy, gx, 0.0, np.float32(1.0 / ((2 * ry + 1) * (2 * rx + 1))), (sy, sx), kind)
    return SpatialFilter(-gy, gx, 1.0, 0.0, (sy, sx), kind)


def as_filter(filt_or_sigma, kind="bandpass", radius=None):
    """``filt_or_sigma`` as a SpatialFilter: itself, or spatial_filter(sigma, kind, radius)."""
    if isinstance(filt_or_sigma, SpatialFilter):
        return filt_or_sigma
    return spatial_filter(filt_or_sigma, kind, radius)


def reflect_index(i, d):
    """refl(i) for indices in [-d, 2 d): -1 - i below 0, 2 d - 1 - i from d on."""
    i = np.asarray(i, dtype=np.int64)
    return np.where(i < 0, -1 - i, np.where(i >= d, 2 * d - 1 - i, i))


def _out_dtype(dtype):
    try:
        key = np.dtype("float32" if dtype is None else dtype).name
    except TypeError:
        key = None
    if key not in _OUT_DTYPES:
        raise ValueError("dtype must be None or one of {}, got {!r}".format(_OUT_DTYPES, dtype))
    return np.dtype(key)


def _chain(planes, w=None):
    """The chain over ``planes`` (a list of float32 arrays, one per tap), ascending: acc = fl(w[0] p_0), acc = fl(acc +
    fl(w[j] p_j)); without weights the plain adds.  NumPy's float32 arithmetic rounds every operation on its own."""
    acc = planes[0].copy() if w is None else w[0] * planes[0]
    for j in range(1, len(planes)):
        acc = acc + (planes[j] if w is None else w[j] * planes[j])
    return acc


def filter_frames(frames, filt, dtype=None):
    """pmd_spatial_filter on the host, with its bits: ``frames`` (n, d1, d2) or (d1, d2), float32 / uint16 / int16 (other
    dtypes are converted to float32 first), filtered by ``filt`` (a SpatialFilter, or a sigma: band-pass) into ``dtype``
    (None: float32)."""
    from .export import quantize

    filt = as_filter(filt)
    f = np.asarray(frames)
    single = f.ndim == 2
    if single:
        f = f[None]
    if f.ndim != 3:
        raise ValueError("frames must have shape (n, d1, d2) or (d1, d2), got {}".format(f.shape))
    n, d1, d2 = f.shape
    filt.check_frame(d1, d2)
    out_dtype = _out_dtype(dtype)
    ry, rx = filt.ry, filt.rx
    yi, xi = reflect_index(np.arange(-ry, d1 + ry), d1), reflect_index(np.arange(-rx, d2 + rx), d2)
    out = np.empty((n, d1, d2), out_dtype)
    centre, box = np.float32(filt.centre), np.float32(filt.box)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(n):
            a = f[k].astype(np.float32)
            p = a[:, xi]                                                    # (d1, d2 + 2 rx): the reflected columns
            taps = [p[:, j:j + d2] for j in range(2 * rx + 1)]
            h = _chain(taps, filt.wx)[yi]                                   # (d1 + 2 ry, d2): the reflected rows
            g = _chain([h[i:i + d1] for i in range(2 * ry + 1)], filt.wy)
            v = g if centre == 0 else centre * a + g
            if box != 0:
                s = _chain(taps)[yi]
                v = v - box * _chain([s[i:i + d1] for i in range(2 * ry + 1)])
            out[k] = quantize(v.astype(np.float32), out_dtype)
    return out[0] if single else out


# ---- device side ----------------------------------------------------------------------------------------------------
def run_filter(ctx, filt, X, elem, n, d1, d2, out, out_elem=0):
    """Enqueue pmd_spatial_filter on n contiguous d1 x d2 frames at device address X into contiguous frames at ``out``."""
    D = d1 * d2
    ctx.call("pmd_spatial_filter", X, int(elem), D, d2, int(n), d1, d2, filt.ry, filt.rx,
             C.c_void_p(filt.wy.ctypes.data), C.c_void_p(filt.wx.ctypes.data), filt.centre, filt.box, out, int(out_elem), D,
             d2)


def filter_image(ctx, filt, image):
    """One (d1, d2) float32 image filtered on the device with the kernel (n = 1), back on the host as float32."""
    import torch

    d1, d2 = image.shape
    src = torch.from_numpy(np.array(image, dtype=np.float32, order="C")).to(ctx.device)
    dst = torch.empty_like(src)
    run_filter(ctx, filt, C.c_void_p(src.data_ptr()), 0, 1, d1, d2, C.c_void_p(dst.data_ptr()))
    return dst.cpu().numpy()


def filter_device_bytes(*, d1, d2, nb, esize, host_source, n_batches, out_esize=4, host_dest=False):
    """Device bytes filter_movie holds on d1 x d2 frames read in batches of nb: the frame batches (two for a host source
    of more than one batch) and, for a host destination, the output ring of two blocks.  No term grows with the movie's
    length."""
    need = batch_buffer_bytes(nb, d1 * d2, esize, host_source, n_batches)
    if host_dest:
        need += HOST_SLOTS * min(BLOCK, nb) * d1 * d2 * out_esize
    return need + (1 << 20)


def filter_movie(movie, out, filt_or_sigma, *, kind="bandpass", radius=None, dtype=None, frame_batch_size=10000,
                 num_workers=0, bigtiff=None, device=None, ctx=None):
    """Write every frame of ``movie`` ((T, d1, d2); the sources of export_movie) filtered by ``filt_or_sigma`` (a
    SpatialFilter, or a sigma / pair of sigmas for spatial_filter(sigma, kind, radius)) to ``out`` (the destinations of
    export_movie: a .tif / .tiff or .npy path, a host array, a contiguous device tensor).  ``dtype``: "float32" (None),
    "uint16", "int16" (round half to even, saturating, NaN -> 0).  Returns the path or the array.

    The movie is read once, in the frame batches of the streamed decomposition; every output bit is that of
    filter_frames, whatever the frame_batch_size, source and destination.  Device memory does not grow with the movie's
    length (filter_device_bytes is checked before anything is allocated).  Argument errors are raised before any device
    work and before a file is created; a file this call created is removed when it fails midway.  ``out`` must not share
    memory with the movie."""
    from .register import _check_no_alias, _movie_info

    info = _movie_info(movie)
    T, d1, d2, on_device, np_dtype = info
    if T < 1:
        raise ValueError("the movie has no frames")
    filt = as_filter(filt_or_sigma, kind, radius)
    filt.check_frame(d1, d2)
    if not _is_int(frame_batch_size) or frame_batch_size < 1:
        raise ValueError("frame_batch_size must be an int >= 1, got {!r}".format(frame_batch_size))
    check_bigtiff(bigtiff)
    out_dtype = _out_dtype(dtype)
    if out is None:
        raise TypeError("filter_movie needs a destination")
    _check_no_alias(movie, out)
    dest = _destination(out, (T, d1, d2), out_dtype, bigtiff, device_index(None, device, ctx))
    plan = block_plan(T, int(frame_batch_size))
    nb = plan[0][1] - plan[0][0]
    with device_context(None, device, ctx) as (ctx, _):
        need = filter_device_bytes(d1=d1, d2=d2, nb=nb, esize=np_dtype.itemsize, host_source=not on_device,
                                   n_batches=len(plan), out_esize=out_dtype.itemsize, host_dest=dest.kind != "device")
        check_fit("filter_movie", need, _device_free_bytes(ctx.device))
        out_elem = _ELEM[out_dtype]

        def write(c0, m, yp, elem, at):
            run_filter(ctx, filt, yp, elem, m, d1, d2, at, out_elem)

        return movie_pass(ctx, dest, (d1, d2), out_dtype, max(1, min(BLOCK, nb)),
                          each_block(ctx, movie, plan, d1 * d2, int(frame_batch_size), num_workers), write)
