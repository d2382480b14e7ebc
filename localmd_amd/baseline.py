"""
Rolling-baseline dF/F: a baseline F0 that follows bleaching and slow drift along time, and the movie (or a set of
traces) detrended or normalised by it.

``rolling_baseline(pmd, movie, window=...)`` returns the baseline of every pixel at knots ``temporal_bin`` frames apart;
``dff_movie(pmd, out, movie, window=...)`` writes ``(x - F0) / F0`` (or ``x - F0``, or F0) frame by frame to the
destinations of export_movie; ``trace_baseline(traces, window=...)`` does the same for (K, T) time courses.  A sliding
filter is neither a running reduction nor linear in the movie, so every pixel of every frame is looked at:

1. knots: the means of bins of ``temporal_bin`` frames (``pmd_bin_means``, csrc/baseline.hip), written into a resident
   (n_bins x D) device buffer.  Denoised blocks come from _expand.Expander and read no movie; raw blocks are taken from
   the batch in place, in their own dtype.
2. the sliding minimum over ``2 h + 1`` knots, and for "maximin" (the morphological opening, as in Suite2p) the sliding
   maximum of the result (``pmd_sliding_extremum``, work per knot independent of h), in ranges of pixel columns so that
   the workspace stays within WORK_BYTES.  ``method="percentile"`` takes instead the running low percentile of CaImAN's
   detrend_df_f: the member of rank min(W - 1, floor(q W)) of the W = 2 h + 1 knots around each knot, the series'
   ends replicated (``pmd_sliding_quantile``, exact on integer keys; work per knot grows as min(W, n_bins)).
3. dff_movie only: a second pass rebuilds every block and writes it through ``pmd_baseline_apply``, which interpolates
   the baseline between the knots, into the destination (_sink.movie_pass opens it, gives every block its address and
   orders finish, abort and close; the file is created once the knots stand).  The knots stay on the device between the
   passes.

The bins divide the 1024-frame reconstruction block, so a bin never straddles a block and every output bit is the same
for every frame_batch_size, source and residency.  This is the one consumer whose device memory grows with the movie's
length T: the knots and the filter's output are ``4 D ceil(T / temporal_bin)`` bytes each.  Raise temporal_bin when they
do not fit.
"""
import numpy as np

from . import _stream
from ._expand import KindBlocks, KindPlan, expander_bytes
from ._movie import _device_free_bytes
from ._sink import HOST_SLOTS, _destination, check_bigtiff, device_index, movie_pass
from ._stream import BLOCK, batch_buffer_bytes, check_pmd, device_context

KINDS = ("denoised", "raw")
METHODS = ("maximin", "minimum")      # the sliding extrema
PERCENTILE = "percentile"             # the sliding order statistic
ALL_METHODS = METHODS + (PERCENTILE,)
DEFAULT_Q = 0.08             # CaImAN's detrend_df_f: the 8th percentile
OUTPUTS = ("baseline", "detrended", "dff")
MAX_BIN = 256                # PMD_BASELINE_MAX_BIN: a bin lies inside one reconstruction block
MAX_FRAMES = 1 << 23         # PMD_BASELINE_MAX_FRAMES: frame numbers and bin centres (multiples of 1/2) are exact in fp32
WORK_BYTES = 256 << 20       # the most workspace one pmd_sliding_extremum call gets
QUANTILE_SLICE = 128         # PMD_SLIDING_QUANTILE_SLICE: the outputs one wave of pmd_sliding_quantile walks
MAX_HALF = 1 << 30           # pmd_sliding_quantile: the counts of a window of 2 half + 1 members fit 32 bits


# ---- host side: the knot grid, the filter plan, the interpolation (no device work) ----------------------------------
def half_window(window, temporal_bin):
    """The smallest h >= 0 with (2 h + 1) temporal_bin >= window."""
    return -(-int(window) // int(temporal_bin)) // 2


def bin_centres(T, temporal_bin):
    """The centres c_j = j b + (n_j - 1) / 2 (float64) of the ceil(T / b) bins of T frames; the last bin may be short."""
    T, b = int(T), int(temporal_bin)
    j = np.arange(-(-T // b), dtype=np.int64)
    return j * b + (np.minimum(b, T - j * b) - 1) / 2.0


def interpolate(knots, centres, t):
    """The baseline at the frames ``t`` (integers) from ``knots`` ((n_bins, ...) float32) at ``centres``, with the fp32
    arithmetic of pmd_baseline_apply: K_0 up to the first centre, K_last from the last on, K_j at a centre, else
    K_j + w (K_{j+1} - K_j) with w = (t - c_j) / (c_{j+1} - c_j), every operation rounded to float32 on its own."""
    knots = np.asarray(knots, dtype=np.float32)
    c = np.asarray(centres, dtype=np.float64)
    t = np.asarray(t, dtype=np.int64).reshape(-1)
    nb = len(c)
    j = np.searchsorted(c, t, side="right") - 1              # the last bin whose centre is at or before t
    ja, jb = np.clip(j, 0, nb - 1), np.clip(j + 1, 0, nb - 1)
    inside = (j >= 0) & (j < nb - 1)
    num = (t - c[ja]).astype(np.float32)
    den = np.where(inside, c[jb] - c[ja], 1.0).astype(np.float32)
    w = (num / den).astype(np.float32)
    exact = ~inside | (t == c[ja])
    shape = (-1,) + (1,) * (knots.ndim - 1)
    ka, kb = knots[ja], knots[jb]
    with np.errstate(invalid="ignore", over="ignore"):       # inf - inf and the like: NaN, as on the device
        f = ka + w.reshape(shape) * (kb - ka)
    return np.where(exact.reshape(shape), ka, f).astype(np.float32)


def percentile_rank(half, q):
    """The 0-based rank min(W - 1, floor(q W)) of the q-quantile among the W = 2 half + 1 members of a window, in
    float64: scipy.ndimage.percentile_filter's rule for the percentile 100 q."""
    W = 2 * int(half) + 1
    return min(W - 1, int(np.floor(np.float64(q) * np.float64(W))))


def quantile_work_floats(n_bins, cols, half):
    """pmd_sliding_quantile_work_floats: the state of a column lives in registers, there is no workspace."""
    return 0


def filter_plan(n_bins, N):
    """([(c0, c1), ...], work_floats): the ranges of pixel columns one pmd_sliding_extremum call takes each, multiples
    of 256 columns (of 4 when the series is very long) whose workspace of n_bins * round_up(columns, 4) floats stays
    within WORK_BYTES, and the floats of the largest."""
    n_bins, N = int(n_bins), int(N)
    cols = WORK_BYTES // (4 * n_bins)
    cols = cols // 256 * 256 if cols >= 256 else max(4, cols // 4 * 4)
    cols = min(cols, -(-N // 4) * 4)
    return [(c0, min(N, c0 + cols)) for c0 in range(0, N, cols)], n_bins * cols


def knot_bytes(T, D, temporal_bin, method="maximin", half=0):
    """Device bytes that grow with the movie's length: the knots, the filter's output and its workspace (that of the
    sliding extrema, or for "percentile" that of pmd_sliding_quantile over the same column ranges: none)."""
    n_bins = -(-int(T) // int(temporal_bin))
    ranges, work_floats = filter_plan(n_bins, D)
    if method == PERCENTILE:
        work_floats = max(quantile_work_floats(n_bins, c1 - c0, half) for c0, c1 in ranges)
    return 2 * 4 * n_bins * int(D) + 4 * work_floats


def baseline_device_bytes(*, T, D, temporal_bin, nb, esize, kind, n_cols, rank, n_entries, n_a, n_patches, host_source,
                          n_batches, factors_on_device, host_dest=False, method="maximin", half=0):
    """Device bytes rolling_baseline (and dff_movie: ``host_dest`` adds the output ring of a host destination) holds on
    a movie of T frames of D pixels read in batches of nb frames.  Unlike every other consumer of a decomposition this
    one grows with the movie's length, as T / temporal_bin: the knots are 4 D ceil(T / temporal_bin) bytes, the filter's
    output as much again, and the extremum filters' workspace up to the same, bounded by WORK_BYTES; the percentile
    filter (``method``, ``half``) has none (knot_bytes).  On top of them the batch buffers of a raw pass, or for the
    denoised movie the expander with one expanded block."""
    need = knot_bytes(T, D, temporal_bin, method, half)
    if kind == "raw":
        need += batch_buffer_bytes(nb, D, esize, host_source, n_batches)
    else:
        need += expander_bytes(D=D, n_cols=n_cols, rank=rank, n_entries=n_entries, n_a=n_a, n_patches=n_patches,
                               factors_on_device=factors_on_device, block_panels=1)
    if host_dest:
        need += HOST_SLOTS * BLOCK * D * 4
    return need + (1 << 20)     # the allocator's rounding of the small arrays


def check_fit(what, need, free):
    _stream.check_fit(what, need, free, hint="; the knots grow with the movie's length: raise temporal_bin (or lower "
                                             "frame_batch_size)")


def _check_bin(temporal_bin):
    ok = isinstance(temporal_bin, (int, np.integer)) and not isinstance(temporal_bin, (bool, np.bool_))
    if not ok or not 1 <= int(temporal_bin) <= MAX_BIN or int(temporal_bin) & (int(temporal_bin) - 1):
        raise ValueError("temporal_bin must be a power of two from 1 to {}, got {!r}".format(MAX_BIN, temporal_bin))
    return int(temporal_bin)


def _check_window(window):
    ok = isinstance(window, (int, np.integer)) and not isinstance(window, (bool, np.bool_))
    if not ok or int(window) < 1:
        raise ValueError("window must be a number of frames >= 1, got {!r}".format(window))
    return int(window)


def _check_name(value, allowed, word):
    if not isinstance(value, str) or value not in allowed:
        raise ValueError("unknown {} {!r}; choose from {}".format(word, value, allowed))
    return value


def _check_method(method, q):
    """(method, q): the method's name against ALL_METHODS; q is a float in [0, 1] for "percentile" (None: DEFAULT_Q) and
    None for the others."""
    _check_name(method, ALL_METHODS, "method")
    if method != PERCENTILE:
        if q is not None:
            raise ValueError("q belongs to method 'percentile', the method is {!r}".format(method))
        return method, None
    if q is None:
        return method, DEFAULT_Q
    ok = isinstance(q, (int, float, np.integer, np.floating)) and not isinstance(q, (bool, np.bool_))
    if not ok or not 0.0 <= float(q) <= 1.0:         # a NaN fails both comparisons
        raise ValueError("q must be a number in [0, 1], got {!r}".format(q))
    return method, float(q)


def _check_half(half, method):
    if method == PERCENTILE and half >= MAX_HALF:
        raise ValueError("a window of {} knots is too long for method 'percentile'".format(2 * half + 1))
    return half


def _check_frames(T, what):
    if T == 0:
        raise ValueError("{} has no frames: there is no baseline".format(what))
    if T >= MAX_FRAMES:
        raise ValueError("{} frames are too many: the bin centres are exact in fp32 below 2^23 frames".format(T))


class Baseline:
    """Result of rolling_baseline: ``knots`` ((n_bins, d1, d2) float32, the baseline at the bin centres), ``centres``
    ((n_bins,) float64 frame positions), ``temporal_bin``, ``window_frames`` = (2 h + 1) temporal_bin, ``method``,
    ``kind``, ``n_frames`` and ``q`` (the quantile of method "percentile"; None for the extremum methods)."""

    def __init__(self, knots, temporal_bin, window_frames, method, kind, n_frames, *, q=None):
        self.knots = knots
        self.temporal_bin, self.window_frames = int(temporal_bin), int(window_frames)
        self.method, self.kind, self.n_frames = method, kind, int(n_frames)
        self.q = q
        self.centres = bin_centres(self.n_frames, self.temporal_bin)

    def frames(self, t0=0, t1=None):
        """The baseline of frames t0 .. t1 ((t1 - t0, d1, d2) float32), interpolated on the host with the fp32 formula
        of the device (interpolate): the bits of dff_movie(..., output="baseline")."""
        t1 = self.n_frames if t1 is None else int(t1)
        t0 = int(t0)
        if not 0 <= t0 <= t1 <= self.n_frames:
            raise ValueError("frames {} .. {} lie outside 0 .. {}".format(t0, t1, self.n_frames))
        return interpolate(self.knots, self.centres, np.arange(t0, t1))

    def __repr__(self):
        method = self.method if self.q is None else "{} q={:g}".format(self.method, self.q)
        return "Baseline({}; {} knots of {} frames; {} over {} frames)".format(
            self.kind, len(self.centres), self.temporal_bin, method, self.window_frames)


def _check_baseline(b, shape, kind):
    T, d1, d2 = shape
    if not isinstance(b, Baseline):
        raise TypeError("baseline must be a localmd_amd.Baseline, got {}".format(type(b).__name__))
    if b.kind != kind:
        raise ValueError("the baseline is that of the {} movie, kind is {!r}".format(b.kind, kind))
    _check_bin(b.temporal_bin)
    if b.method == PERCENTILE and b.q is None:
        raise ValueError("a percentile baseline must say its q")
    _check_method(b.method, b.q)
    if b.n_frames != T:
        raise ValueError("the baseline covers {} frames, the decomposition {}".format(b.n_frames, T))
    want = (-(-T // b.temporal_bin), d1, d2)
    k = b.knots
    if not isinstance(k, np.ndarray) or k.dtype != np.float32 or k.shape != want:
        raise ValueError("the baseline's knots must be a float32 array of shape {}".format(want))


# ---- device side ----------------------------------------------------------------------------------------------------
def _offset(t, c0):
    import ctypes as C

    return C.c_void_p(t.data_ptr() + 4 * int(c0))


def _filter(ctx, K, half, method, q=None):
    """The sliding minimum (and for "maximin" then the maximum) over ``2 half + 1`` rows of the (n_bins, N) device
    tensor K, or for "percentile" the sliding member of rank percentile_rank(half, q) in one pass, column range by
    column range; returns the tensor that holds the result (K or the second buffer)."""
    import torch
    from ._lib import ptr

    n_bins, N = (int(x) for x in K.shape)
    ranges, work_floats = filter_plan(n_bins, N)
    src, dst = K, torch.empty_like(K)
    if method == PERCENTILE:
        rank = percentile_rank(half, q)
        query = ctx.lib.pmd_sliding_quantile_work_floats
        work_floats = max(int(query(n_bins, c1 - c0, int(half))) for c0, c1 in ranges)
        assert work_floats == max(quantile_work_floats(n_bins, c1 - c0, half) for c0, c1 in ranges)   # as check_fit saw
        work = torch.empty(work_floats, dtype=torch.float32, device=K.device) if work_floats else None
        for c0, c1 in ranges:
            ctx.call("pmd_sliding_quantile", _offset(src, c0), N, n_bins, c1 - c0, int(half), rank, _offset(dst, c0), N,
                     ptr(work), work_floats)
        return dst
    work = torch.empty(work_floats, dtype=torch.float32, device=K.device)
    for is_max in ((0, 1) if method == "maximin" else (0,)):
        for c0, c1 in ranges:
            ctx.call("pmd_sliding_extremum", _offset(src, c0), N, n_bins, c1 - c0, int(half), is_max, _offset(dst, c0), N,
                     ptr(work), work_floats)
        src, dst = dst, src
    return src


class _Passes:
    """The two passes of one call over the blocks of ``blocks`` (KindBlocks): a block is the expanded denoised frames in
    fp32, or the batch's own raw frames in place."""

    def __init__(self, ctx, blocks, temporal_bin):
        self.ctx, self.blocks, self.bin = ctx, blocks, temporal_bin
        self.T, self.D = blocks.plan.T, blocks.plan.D

    def run(self, each):
        """each(X, elem, c0, m): the m frames from c0 on of every reconstruction block."""
        self.blocks.run(lambda c0, m, yp, elem, xp: each(yp, elem, c0, m) if xp is None else each(xp, 0, c0, m))

    def knots(self, half, method, q=None):
        """Pass 1 and the filters: the (n_bins, D) device tensor of the filtered knots."""
        import torch
        from ._lib import ptr

        ctx, D = self.ctx, self.D
        K = torch.empty((-(-self.T // self.bin), D), dtype=torch.float32, device=ctx.device)
        self.run(lambda X, elem, c0, m: ctx.call("pmd_bin_means", X, int(elem), D, int(m), D, int(c0), self.bin, ptr(K), D))
        return _filter(ctx, K, half, method, q)

    def apply(self, K, mode, min_baseline, dest, frame_shape):
        """Pass 2: every block through pmd_baseline_apply into the destination (movie_pass); what dest.close() returns."""
        from ._lib import ptr

        ctx, D = self.ctx, self.D

        def write(c0, m, X, elem, out):
            ctx.call("pmd_baseline_apply", X, int(elem), D, int(m), D, int(c0), self.T, self.bin, ptr(K), D, mode,
                     float(min_baseline), out, D)

        return movie_pass(ctx, dest, frame_shape, np.dtype(np.float32), min(self.T, BLOCK),
                          lambda each: self.run(lambda X, elem, c0, m: each(c0, m, X, elem)), write)


def _check_common(pmd, movie, kind, temporal_bin, method, q, frame_batch_size):
    """(temporal_bin, q, KindPlan) of the checked arguments."""
    check_pmd(pmd)
    if kind == "residual":
        raise ValueError("the residual's baseline is about 0 and dF/F of it means nothing; choose from {}".format(KINDS))
    _check_name(kind, KINDS, "kind")
    _, q = _check_method(method, q)
    b = _check_bin(temporal_bin)
    raw = kind == "raw"
    if raw and movie is None:
        raise ValueError("kind 'raw' needs the movie: pass movie=")
    kp = KindPlan(pmd, movie if raw else None, raw=raw, panels=() if raw else ("denoised",),
                  frame_batch_size=frame_batch_size)
    _check_frames(kp.T, "the decomposition")
    return b, q, kp


def _fit(what, kp, dv, kind, b, host_dest, free, method, half):
    """check_fit before anything is allocated on the device."""
    check_fit(what, baseline_device_bytes(**kp.facts(dv), T=kp.T, temporal_bin=b, kind=kind, host_dest=host_dest,
                                          method=method, half=half), free)


# ---- public entry points -------------------------------------------------------------------------------------------
def rolling_baseline(pmd, movie=None, *, kind="denoised", window, temporal_bin=16, method="maximin", q=None,
                     frame_batch_size=10000, num_workers=0, device=None, ctx=None):
    """The rolling baseline of every pixel of the ``kind`` movie ("denoised": ``mean_img + var_img * (U R diag(s) Vt)``,
    which reads no movie; "raw": ``movie``, read once; the residual has no baseline to speak of and is refused), as a
    Baseline whose ``knots`` are (n_bins, d1, d2) float32 on the host.

    The series of a pixel is averaged over bins of ``temporal_bin`` frames (a power of two from 1 to 256; bins start at
    frame 0, the last may be short; each mean is an fp32 chain in frame order divided by the count).  ``method``
    "minimum" takes the minimum of the bin means over the 2 h + 1 bins around each bin, the window cut at both ends of
    the series; "maximin" (the default, the morphological opening) then takes the maximum of that over the same window,
    so that a baseline under transients shorter than the window is not pulled below the signal's floor.  ``window`` is
    in frames; h is the smallest integer with (2 h + 1) temporal_bin >= window, and the result says what was used in
    ``window_frames``.  NaN bin means are ignored unless a whole window is NaN.

    ``method`` "percentile" is the running low percentile of CaImAN's detrend_df_f instead: of the W = 2 h + 1 bin means
    around each bin, ordered, the one at the 0-based rank min(W - 1, floor(q W)) (scipy.ndimage.percentile_filter's
    rule for the percentile 100 q), with ``q`` a float in [0, 1], None meaning 0.08; ``q`` with another method is an
    error.  Here the series' ends are replicated, not cut (scipy's mode "nearest"), so every window has W members;
    the order is that of quantile_images, -0 before +0 and every NaN last, so a NaN comes out only where NaNs reach
    down to the rank.  It is exact and bit-reproducible, and unlike an extremum not biased by the knots' noise; its work
    per pixel grows as n_bins min(W, n_bins) where the extrema take n_bins, so temporal_bin=1 with a long window (that
    is CaImAN's filter on the frames themselves) is expensive.  The result carries ``q``.

    Sources, batching and residency are those of summary_images; the knots have the same bits for every
    frame_batch_size, source and residency.  Device memory grows with the movie's length: 8 D ceil(T / temporal_bin)
    bytes of knots and filter output plus, for the extrema, a workspace of up to 256 MB (baseline_device_bytes); a plan
    that does not fit raises ValueError and says to raise temporal_bin.  Argument errors are raised before any device
    work."""
    window = _check_window(window)
    b, q, kp = _check_common(pmd, movie, kind, temporal_bin, method, q, frame_batch_size)
    half = _check_half(half_window(window, b), method)
    T, d1, d2 = (int(x) for x in pmd.shape)
    with device_context(pmd, device, ctx) as (ctx, dv):
        _fit("rolling_baseline", kp, dv, kind, b, False, _device_free_bytes(ctx.device), method, half)
        ps = _Passes(ctx, KindBlocks(ctx, pmd, dv, kp, num_workers), b)
        K = ps.knots(half, method, q)
        ctx.sync()
        knots = K.cpu().numpy().reshape(-1, d1, d2)
    return Baseline(knots, b, (2 * half + 1) * b, method, kind, T, q=q)


def dff_movie(pmd, out, movie=None, *, kind="denoised", output="dff", baseline=None, window=None, temporal_bin=16,
              method="maximin", q=None, min_baseline=0.0, frame_batch_size=10000, num_workers=0, bigtiff=None,
              device=None, ctx=None):
    """Write the ``kind`` movie ("denoised" or "raw") relative to its rolling baseline F0 to ``out`` (the destinations of
    export_movie: a .tif / .tiff or .npy path, a host array, a contiguous device tensor), (T, d1, d2) float32:
    ``output`` "dff" is (x - F0) / F0, 0 where F0 > ``min_baseline`` does not hold (a NaN F0 included); "detrended" is
    x - F0; "baseline" is F0 itself.  Returns the path or the array.

    F0 at a frame is interpolated linearly (fp32, every operation rounded on its own) between the knots of
    rolling_baseline at the bin centres, and constant before the first and after the last centre.  The knots are built
    with ``window``, ``temporal_bin``, ``method`` and ``q`` as in rolling_baseline, or taken from ``baseline``, a Baseline
    of this decomposition and kind, of any method (then ``window`` and ``q`` must be None; its bin and method apply and
    no filter runs).  They stay on the device
    while a second pass rebuilds every block and writes it out: the raw movie is read twice, the denoised movie never.
    Every output bit is the same for every frame_batch_size, source, destination and residency.  Argument errors are
    raised before any device work and before a file is created; a file this call created is removed when it fails
    midway.  Device memory grows with the movie's length as in rolling_baseline."""
    _check_name(output, OUTPUTS, "output")
    if baseline is None:
        if window is None:
            raise ValueError("dff_movie needs window= (in frames) or baseline=")
        window = _check_window(window)
    elif window is not None:
        raise ValueError("pass window= or baseline=, not both")
    check_bigtiff(bigtiff)
    try:
        min_baseline = float(min_baseline)
    except (TypeError, ValueError):
        raise ValueError("min_baseline must be a number, got {!r}".format(min_baseline)) from None
    if baseline is not None and not isinstance(baseline, Baseline):
        raise TypeError("baseline must be a localmd_amd.Baseline, got {}".format(type(baseline).__name__))
    if baseline is not None:
        if q is not None:
            raise ValueError("pass q= with window=, not with baseline=: the baseline has its own")
        temporal_bin, method, q = baseline.temporal_bin, baseline.method, baseline.q
    b, q, kp = _check_common(pmd, movie, kind, temporal_bin, method, q, frame_batch_size)
    T, d1, d2 = (int(x) for x in pmd.shape)
    if baseline is not None:
        _check_baseline(baseline, (T, d1, d2), kind)
        half = 0                             # no filter runs
    else:
        half = _check_half(half_window(window, b), method)
    dev_index = device_index(pmd, device, ctx)
    dest = _destination(out, (T, d1, d2), np.dtype(np.float32), bigtiff, dev_index)
    mode = OUTPUTS.index(output)

    with device_context(pmd, dev_index, ctx) as (ctx, dv):
        _fit("dff_movie", kp, dv, kind, b, dest.kind != "device", _device_free_bytes(ctx.device), method, half)
        ps = _Passes(ctx, KindBlocks(ctx, pmd, dv, kp, num_workers), b)
        if baseline is None:
            K = ps.knots(half, method, q)
        else:
            import torch

            K = torch.from_numpy(np.ascontiguousarray(baseline.knots).reshape(-1, d1 * d2)).to(ctx.device)
        return ps.apply(K, mode, min_baseline, dest, (d1, d2))


def trace_baseline(traces, *, window, temporal_bin=16, method="maximin", q=None, output="dff", min_baseline=0.0,
                   device=None, ctx=None):
    """The rows of ``traces`` ((K, T), for instance those of extract_traces) relative to their rolling baseline:
    (K, T) float32, ``output`` "dff", "detrended" or "baseline" as in dff_movie, the baseline built with ``window``,
    ``temporal_bin``, ``method`` and ``q`` as in rolling_baseline (``temporal_bin=1, method="percentile"`` is CaImAN's
    percentile filter on the frames themselves).  The three kernels of dff_movie run on the transposed
    (T, K) matrix in 1024-frame blocks, so a trace gets the bits the same series gets as a pixel of a movie."""
    import torch
    from ._lib import ptr

    window = _check_window(window)
    b = _check_bin(temporal_bin)
    _, q = _check_method(method, q)
    mode = OUTPUTS.index(_check_name(output, OUTPUTS, "output"))
    min_baseline = float(min_baseline)
    a = np.asarray(traces)
    if a.ndim != 2 or a.dtype.kind not in "iuf" or a.shape[0] < 1:
        raise ValueError("traces must be a (K, T) array of numbers with K >= 1")
    Kn, T = (int(x) for x in a.shape)
    _check_frames(T, "a trace")
    half = _check_half(half_window(window, b), method)
    with device_context(None, device, ctx) as (ctx, _):
        X = torch.from_numpy(np.ascontiguousarray(a.T, dtype=np.float32)).to(ctx.device)
        knots = torch.empty((-(-T // b), Kn), dtype=torch.float32, device=ctx.device)
        blocks = [(c0, min(T, c0 + BLOCK) - c0) for c0 in range(0, T, BLOCK)]
        for c0, m in blocks:
            ctx.call("pmd_bin_means", ptr(X[c0]), 0, Kn, m, Kn, c0, b, ptr(knots), Kn)
        knots = _filter(ctx, knots, half, method, q)
        out = torch.empty((T, Kn), dtype=torch.float32, device=ctx.device)
        for c0, m in blocks:
            ctx.call("pmd_baseline_apply", ptr(X[c0]), 0, Kn, m, Kn, c0, T, b, ptr(knots), Kn, mode, min_baseline,
                     ptr(out[c0]), Kn)
        ctx.sync()
        return np.ascontiguousarray(out.cpu().numpy().T)
