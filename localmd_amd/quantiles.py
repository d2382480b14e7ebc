"""
Quantile images of a movie: exact per-pixel order statistics over time, the median image, the baseline image F0 (a low
percentile, the denominator of every dF/F) and the MAD noise image.

``quantile_images(pmd, movie, kinds=..., q=..., mad=...)`` returns (Q, d1, d2) images of the raw movie, the denoised
movie ``mean + std * (U R diag(s) Vt)`` and their difference.  None of them is a running reduction, and sorting the
movie along time needs all of it at once; on the device an exact answer is a radix select over per-pixel histograms
(csrc/quantile.hip), with memory that does not grow with the movie's length:

* every fp32 value is mapped to an order-preserving 32-bit key (float_keys); a pass over the movie counts, per pixel,
  the 256 values of one 8-bit digit of the keys that agree with the digits found so far
  (``pmd_pixel_hist_accumulate``, the whole batch in one call), and ``pmd_pixel_hist_select`` then picks the bin that
  holds the rank looked for.  Four passes, most significant digit first, leave the key of the order statistic.
* raw: the batch goes to the kernel in place and in its own dtype.  denoised and residual: the 1024-frame blocks are
  expanded on the device by _expand.Expander, as in summary_images, and the expanded block goes to the same kernel as a
  batch of P D pixels.
* the first pass counts every element, so one histogram per kind serves every rank; later passes count once per
  distinct rank, on the batch already on the device.
* the host turns the keys back into floats (key_floats) and finishes the interpolation in float64 (finish_linear).

The device only counts integers, so every output bit is the same for every batching, source and residency.
"""
import numpy as np

from ._expand import KindBlocks, KindPlan, expander_bytes, interleave, split_panels
from ._movie import _device_free_bytes
from ._stream import batch_buffer_bytes, check_fit, check_pmd, device_context, name_tuple, upload_f32
from .maps import KINDS

INTERPOLATIONS = ("linear", "lower", "higher", "nearest")
MAD_TO_STD = 1.4826          # std of a normal variable = MAD_TO_STD * its MAD
GROUP, BINS = 64, 256        # pixels per histogram group, bins per pixel (csrc/quantile.hip)


class Quantiles:
    """Result of quantile_images: ``denoised``, ``raw``, ``residual`` ((Q, d1, d2) float32, or None when not asked
    for), ``mad`` (dict kind -> (d1, d2) float32, or None without mad=True), ``q`` and ``interpolation``."""

    def __init__(self, denoised=None, raw=None, residual=None, mad=None, q=(), interpolation="linear"):
        self.denoised, self.raw, self.residual, self.mad = denoised, raw, residual, mad
        self.q, self.interpolation = tuple(q), interpolation

    def __repr__(self):
        have = [k for k in KINDS if getattr(self, k) is not None]
        return "Quantiles({}; q={}; {}{})".format(", ".join(have), self.q, self.interpolation,
                                                 "; mad" if self.mad is not None else "")


# ---- host side: keys, positions, the finish (no device work) --------------------------------------------------------
def float_keys(x):
    """The uint32 keys of the float32 values ``x``, in the order of np.sort: ~bits for values with the sign bit set,
    bits | 0x80000000 for the others, 0xFFFFFFFF for every NaN (-0 before +0, NaN last)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    return np.where(np.isnan(x), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def key_floats(k):
    """The float32 values of the uint32 keys ``k`` (the inverse of float_keys; 0xFFFFFFFF gives a NaN)."""
    k = np.ascontiguousarray(k, dtype=np.uint32)
    b = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    return b.view(np.float32)


def check_q(q):
    """``q``, a float or a sequence of floats in [0, 1] (duplicates allowed), as a tuple of floats."""
    if isinstance(q, (str, bytes, bool, np.bool_)):
        raise ValueError("q must be a number or a sequence of numbers in [0, 1], got {!r}".format(q))
    try:
        a = np.asarray(q)
    except Exception:
        raise ValueError("q must be a number or a sequence of numbers in [0, 1], got {!r}".format(q)) from None
    if a.dtype.kind not in "iuf" or a.ndim > 1:
        raise ValueError("q must be a number or a sequence of numbers in [0, 1], got {!r}".format(q))
    a = a.reshape(-1).astype(np.float64)
    if a.size == 0:
        raise ValueError("q is empty")
    if not np.all((a >= 0.0) & (a <= 1.0)):          # a NaN fails both comparisons
        raise ValueError("q must lie in [0, 1], got {!r}".format(q))
    return tuple(float(x) for x in a)


def positions(q, T):
    """(h, lo, hi, nearest) for the quantiles ``q`` of T >= 1 values: h = q (T - 1) in float64, lo = floor(h),
    hi = ceil(h), nearest = h rounded half to even, as np.quantile does."""
    h = np.asarray(q, dtype=np.float64) * (int(T) - 1)
    return h, np.floor(h).astype(np.int64), np.ceil(h).astype(np.int64), np.rint(h).astype(np.int64)


def finish_linear(lo, hi, frac):
    """float32(lo + (hi - lo) frac), formed in float64 and rounded once."""
    lo64, hi64 = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    with np.errstate(invalid="ignore"):                # inf - inf, inf * 0: NaN, as in NumPy
        return (lo64 + (hi64 - lo64) * frac).astype(np.float32)


def _needed(q, T, interpolation):
    """Per quantile the ranks it is finished from: (lo, hi, frac) under "linear", (rank, rank, 0) otherwise."""
    h, lo, hi, near = positions(q, T)
    if interpolation == "linear":
        return [(int(a), int(b), float(x - a)) for x, a, b in zip(h, lo, hi)]
    pick = {"lower": lo, "higher": hi, "nearest": near}[interpolation]
    return [(int(a), int(a), 0.0) for a in pick]


def movie_passes(esize, kinds, mad=False):
    """How often quantile_images reads the movie: four times per selection round, one round for the quantiles and one
    more for the MAD; three times in the quantile round when the source is uint16 / int16 (``esize`` 2) and no
    "residual" is asked for; not at all when only "denoised" is asked for."""
    kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
    if tuple(kinds) == ("denoised",):
        return 0
    return (3 if esize == 2 and "residual" not in kinds else 4) + (4 if mad else 0)


def quantile_device_bytes(*, D, nb, esize, n_raw, n_expand, n_pos, centred, n_cols, rank, n_entries, n_a, n_patches,
                          needs_movie, host_source, n_batches, factors_on_device):
    """Device bytes quantile_images holds on a movie of D pixels read in batches of nb frames for n_pos distinct ranks;
    no term grows with the movie's length.  Per kind and rank 1 KB of histogram per pixel (groups of 64 pixels) with 8
    bytes of rank and prefix, the centring vector of a MAD round, the batch buffers, and for the n_expand expanded panels
    one expanded block with the coefficient block and tables of pmd_group_expand, the mean and std images, one block of
    Vt columns, and R s unless the PMDArray already holds it on the device."""
    def state(N):
        return n_pos * (4 * BINS * GROUP * (-(-N // GROUP)) + 8 * N) + (4 * N if centred else 0)

    need = (state(D) if n_raw else 0) + (state(n_expand * D) if n_expand else 0)
    if needs_movie:
        need += batch_buffer_bytes(nb, D, esize, host_source, n_batches)
    if n_expand:
        need += expander_bytes(D=D, n_cols=n_cols, rank=rank, n_entries=n_entries, n_a=n_a, n_patches=n_patches,
                               factors_on_device=factors_on_device, block_panels=n_expand)
    return need + (1 << 20)     # the allocator's rounding of the small arrays


# ---- public entry point --------------------------------------------------------------------------------------------
def quantile_images(pmd, movie=None, *, kinds="denoised", q=0.5, mad=False, interpolation="linear",
                    frame_batch_size=10000, num_workers=0, device=None, ctx=None):
    """Per-pixel quantile images over the frames: ``kinds`` is any non-empty subset of "denoised" (of ``mean_img +
    var_img * (U R diag(s) Vt)``), "raw" (of ``movie``) and "residual" (of raw - denoised); ``q`` a float or a sequence
    of floats in [0, 1] (duplicates allowed, the output keeps the caller's order).  Returns a Quantiles object whose
    ``denoised`` / ``raw`` / ``residual`` are (Q, d1, d2) float32 images in natural orientation, Q = len(q) (None for
    kinds not asked for).

    With h = q (T - 1) in float64 the order statistics lo = floor(h) and hi = ceil(h) of the pixel's T fp32 values are
    found exactly.  ``interpolation``: "lower" returns y(lo), "higher" y(hi), "nearest" y(h rounded half to even), and
    "linear" (the default, as in NumPy) float32(y(lo) + (y(hi) - y(lo)) (h - floor(h))), formed in float64 on the host
    and rounded once.  NaN sorts last, as in np.sort; -0 sorts before +0.

    ``mad=True`` adds ``mad``: per kind the median (always "linear") of |y - m|, m the kind's float32 "linear" median
    image, the difference one fp32 subtraction per element.  It is the raw median absolute deviation: multiply by
    MAD_TO_STD = 1.4826 for the std of normal noise.

    ``movie`` (of ``pmd.shape``; not needed, and never touched, when only "denoised" is asked for): the sources of
    summary_images, read in ``frame_batch_size`` batches, uint16 / int16 in their own dtype.  A selection round is four
    passes over the movie, one per 8-bit digit of the keys; the quantiles take one round and the MAD one more.  The
    float of a 16-bit integer has its low 8 mantissa bits zero, so the last digit of its key is known (0x00, or 0xFF
    for a negative value) and a uint16 / int16 source without "residual" takes three passes in the quantile round: the
    movie is read movie_passes(...) times in all, 3 or 4, plus 4 with mad=True.  After ``pmd.to_device()`` its context
    and uploaded factors are reused.  Every image has the same bits for every frame_batch_size, source and residency,
    for every order and subset of kinds and q.  Argument errors are raised before any device work and before the movie
    is read; a decomposition of no frames has no order statistics and raises ValueError.  A plan that does not fit the
    free device memory raises ValueError (1 KB per pixel, kind and distinct rank)."""
    check_pmd(pmd)
    kinds = name_tuple(kinds, KINDS, "kind", "kinds")
    q = check_q(q)
    if not isinstance(interpolation, str) or interpolation not in INTERPOLATIONS:
        raise ValueError("unknown interpolation {!r}; choose from {}".format(interpolation, INTERPOLATIONS))
    if not isinstance(mad, (bool, np.bool_)):
        raise ValueError("mad must be True or False, got {!r}".format(mad))
    mad = bool(mad)
    if kinds != ("denoised",) and movie is None:
        raise ValueError("kinds {} need the movie: pass movie=".format(kinds))
    kp = KindPlan(pmd, movie, raw="raw" in kinds, panels=tuple(k for k in ("denoised", "residual") if k in kinds),
                  frame_batch_size=frame_batch_size)
    T, d1, d2 = kp.T, kp.d1, kp.d2
    if T == 0:
        raise ValueError("the decomposition has no frames: their order statistics do not exist")
    if T >= 2 ** 31:
        raise ValueError("quantile_images counts in int32: {} frames are too many".format(T))
    need = _needed(q, T, interpolation)
    median = _needed((0.5,), T, "linear")[0]
    ranks = sorted({r for lo, hi, _ in need + ([median] if mad else []) for r in (lo, hi)})

    with device_context(pmd, device, ctx) as (ctx, dv):
        nbytes = quantile_device_bytes(**kp.facts(dv), n_raw=int(kp.raw), n_expand=len(kp.panels), n_pos=len(ranks),
                                       centred=mad, needs_movie=kp.reads_movie)
        check_fit("quantile_images", nbytes, _device_free_bytes(ctx.device))
        run = _Rounds(ctx, KindBlocks(ctx, pmd, dv, kp, num_workers), kp.reads_movie and kp.esize == 2)
        stat = run.select(ranks, None)                               # kind -> (len(ranks), D) float32
        at = {r: i for i, r in enumerate(ranks)}
        out = {k: np.stack([finish_linear(stat[k][at[lo]], stat[k][at[hi]], frac) if hi != lo else stat[k][at[lo]]
                            for lo, hi, frac in need]).reshape(len(q), d1, d2) for k in kinds}
        dev = None
        if mad:
            lo, hi, frac = median
            med = {k: finish_linear(stat[k][at[lo]], stat[k][at[hi]], frac) if hi != lo else stat[k][at[lo]]
                   for k in kinds}
            mranks = sorted({lo, hi})
            stat = run.select(mranks, med)
            dev = {k: (finish_linear(stat[k][0], stat[k][-1], frac) if hi != lo else stat[k][0]).reshape(d1, d2)
                   for k in kinds}
    return Quantiles(mad=dev, q=q, interpolation=interpolation, **out)


class _Select:
    """The state of one selection on N pixels for len(ranks) ranks on the device: hist [ranks][ceil(N / 64)][256][64]
    (zero between passes), rank [ranks][N] int32, prefix [ranks][N] (uint32 bits in int32), and the centring vector."""

    def __init__(self, ctx, N, ranks, centre):
        import torch

        dev = ctx.device
        self.N, self.R = N, len(ranks)
        self.hist = torch.zeros((self.R, -(-N // GROUP) * BINS * GROUP), dtype=torch.int32, device=dev)
        self.rank = torch.tensor(list(ranks), dtype=torch.int32, device=dev).reshape(-1, 1).repeat(1, N)
        self.prefix = torch.zeros((self.R, N), dtype=torch.int32, device=dev)
        self.centre = None if centre is None else upload_f32(ctx, centre)

    def accumulate(self, ctx, Y, elem, n, p):
        from ._lib import ptr

        for j in range(1 if p == 0 else self.R):        # the first pass counts every element: one histogram for all
            ctx.call("pmd_pixel_hist_accumulate", Y, int(elem), self.N, int(n), self.N, ptr(self.centre), int(p),
                     ptr(self.prefix[j]), ptr(self.hist[j]))

    def select(self, ctx, p):
        from ._lib import ptr

        if p == 0 and self.R > 1:
            self.hist[1:] = self.hist[0]
        for j in range(self.R):
            ctx.call("pmd_pixel_hist_select", self.N, ptr(self.hist[j]), ptr(self.rank[j]), ptr(self.prefix[j]))

    def values(self, passes):
        """(ranks, N) float32: the order statistics after ``passes`` passes (3: the keys of 16-bit integers, whose last
        digit is 0x00, or 0xFF under a negative value)."""
        k = self.prefix.cpu().numpy().view(np.uint32)
        if passes == 3:
            k = (k << np.uint32(8)) | np.where(k & np.uint32(0x800000), np.uint32(0), np.uint32(0xFF))
        return key_floats(k)


class _Rounds:
    """The selection rounds of one quantile_images call, over the blocks of ``blocks`` (KindBlocks); ``sixteen``: the
    movie is read as 16-bit integers."""

    def __init__(self, ctx, blocks, sixteen):
        self.ctx, self.blocks, self.sixteen = ctx, blocks, sixteen

    def select(self, ranks, centres):
        """{kind: (len(ranks), D) float32}: the order statistics ``ranks`` of every kind, of |y - centres[kind]| when
        ``centres`` is given."""
        ctx, kp = self.ctx, self.blocks.plan
        D, d1, d2, panels = kp.D, kp.d1, kp.d2, kp.panels
        P = len(panels)
        raw = expanded = None
        raw_passes = 3 if self.sixteen and centres is None else 4
        if kp.raw:
            raw = _Select(ctx, D, ranks, None if centres is None else centres["raw"])
        if P:
            # the histogram kernel takes the expanded block as a batch of P D "pixels"
            shift = None if centres is None else interleave([centres[k] for k in panels], d1, d2)
            expanded = _Select(ctx, P * D, ranks, shift)

        for p in range(4 if P else raw_passes):
            def whole(Y, elem, b0, n):
                raw.accumulate(ctx, Y, elem, n, p)                   # the whole batch in one call

            def each(c0, m, yp, elem, xp):
                if P:
                    expanded.accumulate(ctx, xp, 0, m, p)

            # a pass that only the denoised panel still needs reads no movie
            do_raw = raw is not None and p < raw_passes
            self.blocks.run(each, batch=whole if do_raw else None, read_movie=do_raw or "residual" in panels)
            if do_raw:
                raw.select(ctx, p)
            if expanded is not None:
                expanded.select(ctx, p)
        ctx.sync()

        out = {}
        if raw is not None:
            out["raw"] = raw.values(raw_passes)
        if P:
            out.update(zip(panels, split_panels(expanded.values(4), d1, P, d2)))
        return out
