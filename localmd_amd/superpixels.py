"""
Superpixels: ROI seeds from thresholded local correlations, the step that precedes demixing in the pipeline of the PMD
paper (Buchanan et al. 2018).

``superpixels(pmd, movie, kind=..., th=..., cut_off=...)`` thresholds the movie per pixel at ``median + th * MAD``,
correlates every pixel with its 8 neighbours on the rectified movie, joins neighbours whose correlation exceeds
``cut_off`` and returns the connected components of at least ``min_size`` pixels as a label image, the form of ``rois``
that extract_traces and demix accept: ``pmd.demix(pmd.superpixels().labels)`` needs no ROI from outside.

* the median and MAD images are those of quantile_images (its selection rounds, run in the same context);
* one more pass forms, per pixel, six fp64 sums of the rectified movie y: y, y^2 and y_p y_q for the four forward
  neighbours (``pmd_threshold_moments_accumulate``, csrc/superpixel.hip).  denoised: every 1024-frame block is expanded
  on the device by _expand.Expander and goes to the kernel; raw: the batch in place, in its own dtype.  Every sum is one
  fp64 chain per pixel in frame order, continued over calls, so the bits do not depend on the batching;
* the host finishes the correlations in float64 (finish_correlations) and packs the edges, one byte per pixel;
* ``pmd_grid_components`` labels the components of that graph on the device (union-find, the smaller index as parent);
  the host numbers the kept components and counts their sizes.

Device memory does not grow with the movie's length (superpixel_device_bytes).
"""
import numpy as np

from ._expand import KindBlocks, KindPlan, expander_bytes
from ._movie import _device_free_bytes
from ._stream import batch_buffer_bytes, check_fit, check_pmd, device_context, upload_f32
from .quantiles import movie_passes, quantile_device_bytes, quantile_images

KINDS = ("denoised", "raw")
# bit b of an edge byte joins a pixel to its forward neighbour (di, dj); the four backward neighbours mirror them
FORWARD = ((0, 1), (1, -1), (1, 0), (1, 1))          # E, SW, S, SE
U53 = 2.0 ** -53


class Superpixels:
    """Result of superpixels: ``labels`` ((d1, d2) int32, 0 = none, 1 .. K in ascending order of the component's
    smallest pixel index), ``sizes`` ((K,) int64), ``correlation`` ((d1, d2) float32: the largest correlation with one of
    the 8 neighbours, from 0), ``threshold`` ((d1, d2) float32), ``n_components`` (components before the size filter,
    isolated pixels included), ``edges`` ((d1, d2) uint8: bit 0 E, bit 1 SW, bit 2 S, bit 3 SE) and the arguments
    ``kind``, ``th``, ``cut_off``, ``min_size``, ``max_size``."""

    def __init__(self, labels, sizes, correlation, threshold, n_components, edges, kind, th, cut_off, min_size, max_size):
        self.labels, self.sizes, self.correlation, self.threshold = labels, sizes, correlation, threshold
        self.n_components, self.edges = int(n_components), edges
        self.kind, self.th, self.cut_off, self.min_size, self.max_size = kind, th, cut_off, min_size, max_size

    def __repr__(self):
        return "Superpixels({} of {} components; {}; th={}, cut_off={}, min_size={}, max_size={})".format(
            len(self.sizes), self.n_components, self.kind, self.th, self.cut_off, self.min_size, self.max_size)


# ---- host side (no device work) -------------------------------------------------------------------------------------
def threshold_image(med, mad, th):
    """thr = fl32(fl32(th32 * mad) + med), th32 = float32(th): two fp32 operations on the float32 images."""
    med, mad = np.asarray(med, dtype=np.float32), np.asarray(mad, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.float32(th) * mad).astype(np.float32) + med


def variance_floor(T):
    """3 (T + 2) 2^-53: see finish_correlations."""
    return 3.0 * (int(T) + 2) * U53


def _shifted(a, di, dj, fill=0.0):
    """b[i, j] = a[i + di, j + dj], ``fill`` where that lies outside the image."""
    d1, d2 = a.shape
    b = np.full_like(a, fill)
    i0, i1 = max(0, -di), min(d1, d1 - di)
    j0, j1 = max(0, -dj), min(d2, d2 - dj)
    if i0 < i1 and j0 < j1:
        b[i0:i1, j0:j1] = a[i0 + di:i1 + di, j0 + dj:j1 + dj]
    return b


def finish_correlations(mom, T, d1, d2):
    """(4, d1, d2) float64: the Pearson correlations rho of every pixel p with its forward neighbours q = E, SW, S, SE
    over T frames, from the six sums ``mom`` ((6, d1 d2) float64: S1 = sum y, S2 = sum y^2, Sq = sum y_p y_q):
    rho = (T Sq - S1_p S1_q) / sqrt(var_p var_q) with var = T S2 - S1^2.

    The variance floor.  S1 and S2 are fp64 chains of T non-negative terms (the products are exact), so each carries a
    relative error of at most (T - 1) u, u = 2^-53.  T S2 and S1^2 add one rounding each and their difference one more,
    and S1^2 <= T S2 (Cauchy-Schwarz), so the computed var is within (T + 2 T + 1) u T S2 of the true one to first order:
    var <= 3 (T + 2) u T S2 (variance_floor; the + 2 covers the second-order terms) cannot be told from the variance 0
    of a constant pixel and counts as zero.  A pair that touches such a pixel, or a neighbour outside the image, has
    rho = 0.  Non-finite sums (an infinite value in the movie) give a non-finite rho, which is kept here and makes no edge
    (edge_bytes)."""
    mom = np.asarray(mom, dtype=np.float64).reshape(6, int(d1), int(d2))
    T = float(T)
    S1, S2 = mom[0], mom[1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        var = T * S2 - S1 * S1
        live = ~(var <= variance_floor(T) * T * S2)           # a NaN variance stays live: its rho is NaN
        rho = np.zeros((4, int(d1), int(d2)))
        for b, (di, dj) in enumerate(FORWARD):
            inside = _shifted(np.ones((int(d1), int(d2)), bool), di, dj, False)
            ok = live & _shifted(live, di, dj, False) & inside
            num = T * mom[2 + b] - S1 * _shifted(S1, di, dj)
            den = np.sqrt(np.where(ok, var, 1.0) * np.where(ok, _shifted(var, di, dj), 1.0))
            rho[b] = np.where(ok, num / den, 0.0)
    return rho


def edge_bytes(rho, cut_off):
    """(d1, d2) uint8: bit b is set iff the neighbour lies inside the image and rho[b] is finite and > cut_off."""
    rho = np.asarray(rho, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        on = np.isfinite(rho) & (rho > float(cut_off))
    e = np.zeros(rho.shape[1:], np.uint8)
    for b, (di, dj) in enumerate(FORWARD):
        inside = _shifted(np.ones(rho.shape[1:], bool), di, dj, False)
        e |= (on[b] & inside).astype(np.uint8) << np.uint8(b)
    return e


def correlation_image(rho):
    """(d1, d2) float32: the largest finite rho of a pixel with one of its 8 neighbours, starting from 0."""
    rho = np.asarray(rho, dtype=np.float64)
    r = np.where(np.isfinite(rho), rho, 0.0)
    best = np.zeros(rho.shape[1:])
    for b, (di, dj) in enumerate(FORWARD):
        best = np.maximum(best, r[b])                         # p with its forward neighbour
        best = np.maximum(best, _shifted(r[b], -di, -dj))     # and the pair seen from that neighbour
    return best.astype(np.float32)


def relabel(root, min_size, max_size=None):
    """(labels, sizes, n_components) from the root image (root[c] = smallest pixel index of c's component): components
    with min_size <= size (<= max_size when given) are numbered 1 .. K in ascending order of their root, the rest is 0."""
    root = np.asarray(root)
    roots, inverse, counts = np.unique(root.reshape(-1), return_inverse=True, return_counts=True)
    keep = counts >= int(min_size)
    if max_size is not None:
        keep &= counts <= int(max_size)
    number = np.zeros(len(roots), np.int32)
    number[keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    return number[inverse.reshape(-1)].reshape(root.shape), counts[keep].astype(np.int64), len(roots)


def movie_reads(esize, kind, threshold_given=False):
    """How often superpixels reads the movie (kind "raw") or expands every block of the denoised movie (kind "denoised"):
    once for the moments, and before that the two selection rounds of quantile_images for the median and the MAD unless
    ``threshold`` is given: 8 + 1, and 3 + 4 + 1 for a uint16 / int16 raw movie, whose median round skips the last digit
    while its MAD round, on |y - median|, does not (quantiles.movie_passes)."""
    if threshold_given:
        return 1
    if kind == "denoised":
        return 8 + 1
    return movie_passes(esize, (kind,), mad=True) + 1


def superpixel_device_bytes(*, D, T, nb, esize, kind, threshold_given, n_cols, rank, n_entries, n_a, n_patches, host_source,
                            n_batches, factors_on_device):
    """Device bytes superpixels holds on a movie of D pixels read in batches of nb frames: the larger of its two phases,
    which do not overlap.  The selection rounds of quantile_images (quantile_device_bytes; skipped with ``threshold``),
    and the moments pass: 48 bytes of sums and 4 of threshold per pixel, then 1 byte of edges, 4 of labels and the
    workspace of pmd_grid_components, with the batch buffers (raw) or one expanded block with what the Expander holds
    (denoised).  T only decides whether the median needs one rank or two: no term grows with the movie's length."""
    raw = kind == "raw"
    common = dict(n_cols=n_cols, rank=rank, n_entries=n_entries, n_a=n_a, n_patches=n_patches,
                  factors_on_device=factors_on_device)
    moments = (48 + 4 + 1 + 4) * D + 256
    if raw:
        moments += batch_buffer_bytes(nb, D, esize, host_source, n_batches)
    else:
        moments += expander_bytes(D=D, block_panels=1, **common)
    select = 0
    if not threshold_given:
        select = quantile_device_bytes(D=D, nb=nb, esize=esize, n_raw=int(raw), n_expand=int(not raw),
                                       n_pos=1 if T % 2 else 2, centred=True, needs_movie=raw, host_source=host_source,
                                       n_batches=n_batches, **common)
    return max(moments + (1 << 20), select)


def _check(kind, th, cut_off, min_size, max_size):
    if not isinstance(kind, str) or kind not in KINDS:
        raise ValueError("unknown kind {!r}; choose from {}".format(kind, KINDS))

    def number(x):
        return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_))

    def whole(x):
        return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))

    if not number(th) or not np.isfinite(th):
        raise ValueError("th must be a finite number, got {!r}".format(th))
    if not number(cut_off) or not -1.0 <= cut_off < 1.0:                   # a NaN fails the comparison
        raise ValueError("cut_off must lie in [-1, 1), got {!r}".format(cut_off))
    if not whole(min_size) or min_size < 1:
        raise ValueError("min_size must be an integer >= 1, got {!r}".format(min_size))
    if max_size is not None and (not whole(max_size) or max_size < min_size):
        raise ValueError("max_size must be None or an integer >= min_size, got {!r}".format(max_size))
    return float(th), float(cut_off), int(min_size), None if max_size is None else int(max_size)


# ---- public entry point --------------------------------------------------------------------------------------------
def superpixels(pmd, movie=None, *, kind="denoised", th=2.0, cut_off=0.9, min_size=10, max_size=None, threshold=None,
                frame_batch_size=10000, num_workers=0, device=None, ctx=None):
    """ROI seeds of the movie of ``kind``: "denoised" (of ``mean_img + var_img * (U R diag(s) Vt)``, the default; reads
    no movie) or "raw" (of ``movie``, in its own dtype).  Returns a Superpixels object.  Images are (d1, d2) in natural
    orientation, pixel c = i d2 + j.

    1. thr = fl32(fl32(float32(th) * mad) + med), with med and mad the float32 images of ``quantile_images(pmd, movie,
       kinds=kind, q=0.5, mad=True)``, bit for bit.  ``threshold=`` (a (d1, d2) image) is used as thr instead and the
       selection rounds are skipped.
    2. y = v > thr ? fl32(v - thr) : 0 per element v, in fp32: a NaN value or threshold gives 0.
    3. per pixel the fp64 sums S1 = sum y, S2 = sum y^2 and Sq = sum y_p y_q for the forward neighbours E, SW, S, SE, each
       one chain over the frames in ascending order with exact products.
    4. rho_pq = (T Sq - S1_p S1_q) / sqrt(var_p var_q), var = T S2 - S1^2, in float64 on the host.  A variance at or below
       3 (T + 2) 2^-53 T S2, the rounding of the two chains (finish_correlations), counts as zero; a pair that touches
       such a pixel has rho = 0, and a non-finite rho makes no edge.
    5. neighbours p, q are joined iff rho_pq > ``cut_off`` (in [-1, 1)).
    6. the connected components of ``min_size`` <= size (<= ``max_size`` when given) are numbered 1 .. K in ascending
       order of their smallest pixel index; every other pixel is 0.

    Passes: the moments take one read of the movie (raw) or one expansion of every block (denoised); the median and the
    MAD take the two selection rounds of quantile_images before it: 8 + 1 in all, 3 + 4 + 1 for a uint16 / int16 raw movie
    (movie_reads, quantiles.movie_passes), and 1 with ``threshold=``.

    ``movie`` (of ``pmd.shape``; not needed, and never touched, for "denoised"): the sources of summary_images, read in
    ``frame_batch_size`` batches.  After ``pmd.to_device()`` its context and uploaded factors are reused.  Every result
    has the same bits for every frame_batch_size, source and residency, and for order "C" and "F" of the same movie.
    Argument errors are raised before any device work and before the movie is read; a decomposition of no frames raises
    ValueError, and so does a plan that does not fit the free device memory."""
    check_pmd(pmd)
    th, cut_off, min_size, max_size = _check(kind, th, cut_off, min_size, max_size)
    T, d1, d2 = (int(x) for x in pmd.shape)
    D = d1 * d2
    thr = None
    if threshold is not None:
        thr = np.asarray(threshold)
        if thr.shape != (d1, d2) or thr.dtype.kind not in "iuf":
            raise ValueError("threshold must be a numeric image of shape {}, got {} {}".format((d1, d2), thr.dtype, thr.shape))
        thr = np.ascontiguousarray(thr, dtype=np.float32)
    raw = kind == "raw"
    if raw and movie is None:
        raise ValueError('kind "raw" needs the movie: pass movie=')
    kp = KindPlan(pmd, movie if raw else None, raw=raw, panels=() if raw else ("denoised",),
                  frame_batch_size=frame_batch_size)
    if T == 0:
        raise ValueError("the decomposition has no frames: their correlations do not exist")
    if D >= 2 ** 31:
        raise ValueError("superpixels labels pixels in int32: {} pixels are too many".format(D))

    with device_context(pmd, device, ctx) as (ctx, dv):
        nbytes = superpixel_device_bytes(**kp.facts(dv), T=T, kind=kind, threshold_given=thr is not None)
        check_fit("superpixels", nbytes, _device_free_bytes(ctx.device))
        if thr is None:
            qi = quantile_images(pmd, movie if raw else None, kinds=kind, q=0.5, mad=True, frame_batch_size=frame_batch_size,
                                 num_workers=num_workers, ctx=ctx)
            thr = threshold_image(getattr(qi, kind)[0], qi.mad[kind], th)
        mom = _moments(ctx, KindBlocks(ctx, pmd, dv, kp, num_workers), thr)
        rho = finish_correlations(mom, T, d1, d2)
        edges = edge_bytes(rho, cut_off)
        root = _components(ctx, edges)
    labels, sizes, n_components = relabel(root, min_size, max_size)
    return Superpixels(labels, sizes, correlation_image(rho), thr, n_components, edges, kind, th, cut_off, min_size,
                       max_size)


def _moments(ctx, blocks, thr):
    """(6, D) float64: the sums of pmd_threshold_moments_accumulate over the whole movie."""
    import torch
    from ._lib import ptr

    d1, d2, D = blocks.plan.d1, blocks.plan.d2, blocks.plan.D
    thr_d = upload_f32(ctx, thr.reshape(-1))
    mom = torch.zeros((6, D), dtype=torch.float64, device=ctx.device)

    def accumulate(X, elem, n):
        ctx.call("pmd_threshold_moments_accumulate", X, int(elem), D, int(n), d1, d2, ptr(thr_d), ptr(mom))

    def each(c0, m, yp, elem, xp):
        if xp is not None:                                    # denoised: block by block
            accumulate(xp, 0, m)

    blocks.run(each, batch=lambda Y, elem, b0, n: accumulate(Y, elem, n))     # raw: the batch in place, any length
    ctx.sync()
    return mom.cpu().numpy()


def _components(ctx, edges):
    """(d1, d2) int32: pmd_grid_components of the edge bytes."""
    import torch
    from ._lib import ptr

    d1, d2 = edges.shape
    e = torch.from_numpy(np.ascontiguousarray(edges)).to(ctx.device)
    label = torch.empty((d1, d2), dtype=torch.int32, device=ctx.device)
    nws = int(ctx.lib.pmd_grid_components_workspace_bytes(d1, d2))
    ws = torch.empty(nws, dtype=torch.uint8, device=ctx.device)
    ctx.call("pmd_grid_components", d1, d2, ptr(e), ptr(label), ptr(ws), nws)
    return label.cpu().numpy()
