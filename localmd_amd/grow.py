"""
Growing ROI supports: the step between two demixings in the pipeline of the PMD paper (Buchanan et al. 2018).

``demix`` fits footprints on the supports it is given.  ``grow_rois(pmd, demixed, ...)`` replaces the support of every
ROI by the connected region around it where the movie, with the other ROIs taken out, correlates with the ROI's trace;
``merge_rois`` joins ROIs that then share most of their support and have correlated traces; ``refine_demix`` alternates
the three.

* the window of an ROI is the bounding box of its support ``{p : A[k, p] > 0}``, widened by ``halo`` pixels and clipped;
  every (window pixel, ROI) is a pair (pair_tables), sorted by (ROI, pixel);
* one pass forms, per pair, three fp64 sums over the frames of ``y = x_p - sum_{l != k} A[l, p] c_l`` (fp32, one ROI
  after the other in ascending order): y, y^2 and y c_k (``pmd_roi_window_moments_accumulate``, csrc/roigrow.hip).
  denoised: every 1024-frame block is expanded on the device by _expand.Expander; raw: the block in place in its batch,
  in its own dtype.  Every sum is one fp64 chain per pair in frame order, continued over calls, so the bits do not depend
  on the batching;
* the host finishes correlation and slope in float64 (finish_moments), grows every support on its window
  (grow_support) and takes the slopes as the new footprint values.

Device memory does not grow with the movie's length (grow_device_bytes).
"""
import numpy as np
import scipy.ndimage
import scipy.sparse
import scipy.sparse.csgraph

from ._expand import KindBlocks, KindPlan, expander_bytes
from ._movie import _device_free_bytes
from ._stream import BLOCK, _is_int, batch_buffer_bytes, check_fit, check_pmd, device_context
from .demix import MAX_COVER
from .superpixels import KINDS
from .superpixels import variance_floor as _nonneg_floor

STATUSES = ("grown", "fixed", "lost", "oversize", "empty")
_EIGHT = np.ones((3, 3), dtype=bool)


class Grown:
    """Result of grow_rois.  ``rois`` (scipy.sparse.csr_matrix (K', d1 d2) float32, columns numbering pixels in C order
    like ``Demixed.footprints``, indices ascending: one row per input ROI with a non-empty support), ``source`` ((K',)
    int64: the input row of each output row), ``labels`` ((K',), those of the sources), ``correlation`` (csr (K, d1 d2)
    float32 with an explicit entry, zeros included, for every pixel of every window), ``threshold`` ((K,) float64: the
    threshold the ROI ended on, ``corr_th`` for an ROI that was not grown), ``added`` / ``removed`` ((K,) int64: pixels
    the support gained / lost) and ``status`` ((K,) of STATUSES)."""

    def __init__(self, rois, source, labels, correlation, threshold, added, removed, status):
        self.rois, self.source, self.labels, self.correlation = rois, source, labels, correlation
        self.threshold, self.added, self.removed, self.status = threshold, added, removed, status

    def __repr__(self):
        return "Grown({} of {} ROIs; {})".format(self.rois.shape[0], len(self.status), ", ".join(
            "{} {}".format(int((self.status == s).sum()), s) for s in STATUSES if (self.status == s).any()))


class Merged:
    """Result of merge_rois: ``rois`` (csr (K', D) float32), ``labels`` ((K',)) and ``groups`` (the ascending input rows
    of every output row, a list of K' int64 arrays)."""

    def __init__(self, rois, labels, groups):
        self.rois, self.labels, self.groups = rois, labels, groups

    def __repr__(self):
        return "Merged({} ROIs from {})".format(len(self.groups), sum(len(g) for g in self.groups))


class Refined:
    """Result of refine_demix: ``demixed`` (the last Demixed) and ``rounds`` (a list of (Grown, Merged or None), one per
    round that ran)."""

    def __init__(self, demixed, rounds):
        self.demixed, self.rounds = demixed, rounds

    def __repr__(self):
        return "Refined({!r}, {} rounds)".format(self.demixed, len(self.rounds))


# ---- host side (no device work) -------------------------------------------------------------------------------------
def variance_floor(T):
    """3 (T + 2) 2^-53, the floor of superpixels.variance_floor, for a signed column y of T frames.

    Sy and Syy are fp64 chains of T terms with exact products.  Syy has non-negative terms: its relative error is at
    most (T - 1) u, u = 2^-53.  Sy has signed terms, so its error is bounded absolutely, by (T - 1) u sum|y|, and
    |Sy| <= sum|y| <= sqrt(T Syy) (Cauchy-Schwarz): the error of Sy^2 is at most 2 |Sy| (T - 1) u sum|y| + u Sy^2
    <= (2 T - 1) u T Syy.  T Syy adds one rounding to Syy's error, T u T Syy in all, and the difference one more, at most
    u T Syy: the computed T Syy - Sy^2 is within (T + 2 T - 1 + 1) u T Syy of the true one to first order, and
    3 (T + 2) u T Syy covers the second-order terms.  A variance at or below that cannot be told from the variance 0 of a
    constant column."""
    return _nonneg_floor(T)


def supports(A):
    """The K x D boolean CSR matrix of the supports ``{p : A[k, p] > 0}``, indices ascending."""
    A = scipy.sparse.csr_matrix(A)
    S = scipy.sparse.csr_matrix((A.data > 0, A.indices.copy(), A.indptr.copy()), shape=A.shape)
    S.eliminate_zeros()                                       # in place: on its own index arrays, not on A's
    S.sort_indices()
    return S


def windows(S, d1, d2, halo):
    """(K, 4) int64: (i0, i1, j0, j1), the bounding box of every support of ``S`` (supports) widened by ``halo`` pixels
    on every side and clipped to the d1 x d2 image, rows i0 .. i1 - 1 and columns j0 .. j1 - 1; all zero for an empty
    support."""
    K = S.shape[0]
    win = np.zeros((K, 4), dtype=np.int64)
    for k in range(K):
        idx = S.indices[S.indptr[k]:S.indptr[k + 1]]
        if idx.size:
            i, j = idx // d2, idx % d2
            win[k] = (max(0, int(i.min()) - halo), min(d1, int(i.max()) + halo + 1),
                      max(0, int(j.min()) - halo), min(d2, int(j.max()) + halo + 1))
    return win


def fixed_mask(K, fixed):
    """(K,) bool from ``fixed``: None, a boolean (K,) or an iterable of distinct row indices in [0, K)."""
    out = np.zeros(K, dtype=bool)
    if fixed is None:
        return out
    f = np.asarray(fixed)
    if f.dtype == bool:
        if f.shape != (K,):
            raise ValueError("a boolean fixed must have shape ({},), got {}".format(K, f.shape))
        return f.copy()
    if f.ndim != 1 or (f.size and f.dtype.kind not in "iu"):
        raise ValueError("fixed must be None, a boolean ({},) or a list of row indices, got {!r}".format(K, fixed))
    f = f.astype(np.int64)
    if f.size and (f.min() < 0 or f.max() >= K):
        raise ValueError("fixed names ROI {}, there are {}".format(int(f.max() if f.max() >= K else f.min()), K))
    out[f] = True
    return out


def roi_status(S, win, fixed, max_window):
    """(K,) of STATUSES before growing: "empty" for an empty support, "fixed" for an ROI of ``fixed`` or one whose window
    has more than ``max_window`` pixels, "grown" (to be decided) for the rest."""
    n = np.diff(S.indptr)
    area = (win[:, 1] - win[:, 0]) * (win[:, 3] - win[:, 2])
    status = np.full(S.shape[0], "grown", dtype="<U8")
    status[fixed | (area > max_window)] = "fixed"
    status[n == 0] = "empty"
    return status


def pair_tables(A, win, movable, d2, max_cover=MAX_COVER):
    """The tables of pmd_roi_window_moments_accumulate for the K x D footprints ``A`` (CSR), the windows ``win`` and the
    (K,) bool ``movable`` (the ROIs that get pairs):

    pair_px  int32 (n_pairs,)      C-order pixel of each pair; the pairs are sorted by (ROI, pixel)
    pair_k   int32 (n_pairs,)      its ROI
    roi_ptr  int64 (K + 1,)        pairs of ROI k: roi_ptr[k] .. roi_ptr[k + 1]
    oth_ptr  int64 (n_pairs + 1,)  others of pair i: oth_ptr[i] .. oth_ptr[i + 1]
    oth_k    int32 (n_others,)     the ROIs l != pair_k[i] with A[l, pair_px[i]] != 0, ascending within a pair, fixed
    oth_a    float32 (n_others,)   ROIs among them, and their values

    ValueError when more than ``max_cover`` ROIs cover one pixel (demix's bound)."""
    A = scipy.sparse.csr_matrix(A)
    K, D = A.shape
    col = scipy.sparse.csc_matrix(A)
    col.eliminate_zeros()
    col.sort_indices()
    cover = np.diff(col.indptr)
    if cover.size and int(cover.max()) > max_cover:
        p = int(np.argmax(cover))
        raise ValueError("pixel {} is covered by {} ROIs, at most {} may overlap on one pixel".format(
            p, int(cover[p]), max_cover))
    px, roi_ptr = [], np.zeros(K + 1, dtype=np.int64)
    for k in range(K):
        if movable[k]:
            i0, i1, j0, j1 = (int(x) for x in win[k])
            px.append((np.arange(i0, i1)[:, None] * d2 + np.arange(j0, j1)[None, :]).reshape(-1))
        roi_ptr[k + 1] = roi_ptr[k] + (px[-1].size if movable[k] else 0)
    pair_px = np.concatenate(px).astype(np.int64) if px else np.zeros(0, np.int64)
    pair_k = np.repeat(np.arange(K), np.diff(roi_ptr))
    n_pairs = pair_px.size
    # every entry of every pair's pixel column, then without the pair's own ROI
    cnt = cover[pair_px]
    start = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    owner = np.repeat(np.arange(n_pairs), cnt)
    pos = col.indptr[pair_px][owner] + (np.arange(start[-1]) - start[owner])
    keep = col.indices[pos] != pair_k[owner]
    oth_ptr = np.concatenate([[0], np.cumsum(np.bincount(owner[keep], minlength=n_pairs))]).astype(np.int64)
    return {"pair_px": pair_px.astype(np.int32), "pair_k": pair_k.astype(np.int32), "roi_ptr": roi_ptr,
            "oth_ptr": oth_ptr, "oth_k": col.indices[pos][keep].astype(np.int32),
            "oth_a": col.data[pos][keep].astype(np.float32)}


def trace_sums(traces):
    """(Sc, Scc), (K,) float64 each: np.sum of the contiguous float64 copy of every trace row and of its squares."""
    K = len(traces)
    Sc, Scc = np.zeros(K), np.zeros(K)
    for k in range(K):
        c = np.ascontiguousarray(traces[k], dtype=np.float64)
        Sc[k], Scc[k] = np.sum(c), np.sum(c * c)
    return Sc, Scc


def finish_moments(mom, T, Sc, Scc):
    """(rho, beta), float64 per pair, from the sums ``mom`` ((3, n) float64: Sy, Syy, Syc) over T frames and the sums Sc,
    Scc of each pair's trace: var_y = T Syy - Sy^2, var_c = T Scc - Sc^2, cov = T Syc - Sy Sc; rho = cov / sqrt(var_y
    var_c) when var_y > variance_floor(T) T Syy and var_c > variance_floor(T) T Scc, else 0 (a NaN variance compares
    false: 0); beta = cov / var_c always, whatever that gives."""
    Sy, Syy, Syc = (np.asarray(m, dtype=np.float64) for m in mom)
    Sc, Scc = np.asarray(Sc, dtype=np.float64), np.asarray(Scc, dtype=np.float64)
    T = float(T)
    with np.errstate(all="ignore"):
        var_y = T * Syy - Sy * Sy
        var_c = T * Scc - Sc * Sc
        cov = T * Syc - Sy * Sc
        ok = (var_y > variance_floor(T) * T * Syy) & (var_c > variance_floor(T) * T * Scc)
        rho = np.where(ok, cov / np.sqrt(np.where(ok, var_y, 1.0) * np.where(ok, var_c, 1.0)), 0.0)
        beta = cov / var_c
    return rho, beta


def grow_support(rho, seed, corr_th, shrink=True, max_size=None):
    """(support, th, status) of one ROI on its window: ``rho`` (h, w) float64, ``seed`` (h, w) bool, the current support.
    Candidates are the pixels with a finite rho > th, th = corr_th at first; the 8-connected components of the candidates
    (scipy.ndimage.label, full 3 x 3 structure) that hold a pixel of the seed are kept and their union is the new support,
    with ``shrink=False`` together with the seed.  Nothing kept: (None, th, "lost").  More than ``max_size`` pixels: th
    goes up by 0.1 and the rule is applied again while th + 0.1 < 1, then (None, th, "oversize")."""
    rho, seed = np.asarray(rho, dtype=np.float64), np.asarray(seed, dtype=bool)
    th = float(corr_th)
    while True:
        with np.errstate(invalid="ignore"):
            cand = np.isfinite(rho) & (rho > th)
        lab, _ = scipy.ndimage.label(cand, structure=_EIGHT)
        hit = np.unique(lab[seed & cand])
        if hit.size == 0:
            return None, th, "lost"
        new = np.isin(lab, hit)
        if not shrink:
            new |= seed
        if max_size is None or int(new.sum()) <= max_size:
            return new, th, "grown"
        if th + 0.1 < 1:
            th = th + 0.1
            continue
        return None, th, "oversize"


def grow_all(A, tabs, win, status, rho, beta, d2, corr_th, shrink, max_size):
    """The growing rule on every ROI whose ``status`` is "grown" so far.  Returns (rows, threshold, added, removed,
    status): rows[k] = (indices, values) of ROI k's new row (int64 ascending, float32), the old one where the ROI keeps
    its support.  New values: float32(beta) on the new support; a pixel kept only through ``shrink=False`` whose beta is
    not > 0 keeps its old value."""
    A = scipy.sparse.csr_matrix(A)
    K = A.shape[0]
    status = status.copy()
    threshold = np.full(K, float(corr_th))
    added, removed = np.zeros(K, np.int64), np.zeros(K, np.int64)
    rows = []
    for k in range(K):
        idx = A.indices[A.indptr[k]:A.indptr[k + 1]].astype(np.int64)
        val = A.data[A.indptr[k]:A.indptr[k + 1]].astype(np.float32)
        on = val > 0
        idx, val = idx[on], val[on]
        order = np.argsort(idx, kind="stable")
        idx, val = idx[order], val[order]
        if status[k] == "grown":
            i0, i1, j0, j1 = (int(x) for x in win[k])
            h, w = i1 - i0, j1 - j0
            p0, p1 = int(tabs["roi_ptr"][k]), int(tabs["roi_ptr"][k + 1])
            local = (idx // d2 - i0) * w + (idx % d2 - j0)
            seed = np.zeros(h * w, dtype=bool)
            seed[local] = True
            new, threshold[k], status[k] = grow_support(rho[p0:p1].reshape(h, w), seed.reshape(h, w), corr_th, shrink,
                                                        max_size)
            if new is not None:
                new = new.reshape(-1)
                old = np.zeros(h * w, dtype=np.float32)
                old[local] = val
                b = beta[p0:p1]
                with np.errstate(invalid="ignore", over="ignore"):
                    v = np.where(seed & ~(b > 0), old, b.astype(np.float32)).astype(np.float32)
                added[k], removed[k] = int((new & ~seed).sum()), int((seed & ~new).sum())
                idx, val = tabs["pair_px"][p0:p1][new].astype(np.int64), v[new]
        rows.append((idx, val))
    return rows, threshold, added, removed, status


def in_pixel_order(rois, fov, order):
    """The sparse (K, d1 d2) ``rois`` whose columns number pixels in C order, as Demixed.footprints and Grown.rois do,
    with its columns in ``order`` ("C": unchanged; "F": the way demix and extract_traces read a sparse matrix on a
    decomposition of order "F")."""
    d1, d2 = (int(x) for x in fov)
    if order == "C":
        return rois
    u_of_c = np.arange(d1 * d2).reshape((d1, d2), order=order).reshape(-1)
    coo = scipy.sparse.coo_matrix(rois)
    out = scipy.sparse.csr_matrix((coo.data, (coo.row, u_of_c[coo.col])), shape=coo.shape)
    out.sort_indices()
    return out


def grow_device_bytes(*, D, nb, esize, n_cols, rank, n_entries, n_a, n_patches, host_source, n_batches, factors_on_device,
                      kind, K, n_pairs, n_others):
    """Device bytes grow_rois holds on a movie of D pixels read in batches of nb frames: per pair 24 bytes of sums and 8
    of indices, 8 (n_pairs + 1) of pointers and 8 bytes per other; one 1024-frame block of the K traces; and the batch
    buffers (raw) or one expanded block with what the Expander holds (denoised).  No term grows with the movie's
    length."""
    need = (24 + 8) * n_pairs + 8 * (n_pairs + 1) + 8 * n_others + 4 * K * BLOCK
    if kind == "raw":
        need += batch_buffer_bytes(nb, D, esize, host_source, n_batches)
    else:
        need += expander_bytes(D=D, block_panels=1, n_cols=n_cols, rank=rank, n_entries=n_entries, n_a=n_a,
                               n_patches=n_patches, factors_on_device=factors_on_device)
    return need + (1 << 20)


def _number(x):
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_))


def _check_grow(kind, corr_th, halo, shrink, max_size, max_window):
    if not isinstance(kind, str) or kind not in KINDS:
        raise ValueError("unknown kind {!r}; choose from {}".format(kind, KINDS))
    if not _number(corr_th) or not -1.0 <= corr_th < 1.0:                  # a NaN fails the comparison
        raise ValueError("corr_th must lie in [-1, 1), got {!r}".format(corr_th))
    if not _is_int(halo) or halo < 0:
        raise ValueError("halo must be an integer >= 0, got {!r}".format(halo))
    if not isinstance(shrink, (bool, np.bool_)):
        raise ValueError("shrink must be True or False, got {!r}".format(shrink))
    if max_size is not None and (not _is_int(max_size) or max_size < 1):
        raise ValueError("max_size must be None or an integer >= 1, got {!r}".format(max_size))
    if not _is_int(max_window) or max_window < 1:
        raise ValueError("max_window must be an integer >= 1, got {!r}".format(max_window))
    return float(corr_th), int(halo), bool(shrink), None if max_size is None else int(max_size), int(max_window)


def _check_demixed(demixed, T, D):
    for name in ("footprints", "traces", "labels", "empty"):
        if not hasattr(demixed, name):
            raise TypeError("demixed must be a localmd_amd.Demixed (footprints, traces, labels, empty), got {}".format(
                type(demixed).__name__))
    if not scipy.sparse.issparse(demixed.footprints):
        raise TypeError("demixed.footprints must be a scipy.sparse matrix")
    A = scipy.sparse.csr_matrix(demixed.footprints)
    C = np.asarray(demixed.traces)
    K = A.shape[0]
    if K < 1 or A.shape != (K, D):
        raise ValueError("demixed.footprints have shape {}, the decomposition needs (K, {})".format(A.shape, D))
    if C.shape != (K, T) or C.dtype.kind != "f":
        raise ValueError("demixed.traces must be a float array of shape {}, got {} {}".format((K, T), C.dtype, C.shape))
    if len(demixed.labels) != K or np.asarray(demixed.empty).shape != (K,):
        raise ValueError("demixed.labels and demixed.empty must have one entry per ROI ({})".format(K))
    if A.nnz and (not np.all(np.isfinite(A.data)) or np.any(A.data < 0)):
        raise ValueError("demixed.footprints hold negative or non-finite values")
    return A.astype(np.float32), np.ascontiguousarray(C, dtype=np.float32)


# ---- public entry points --------------------------------------------------------------------------------------------
def grow_rois(pmd, demixed, movie=None, *, kind="denoised", corr_th=0.6, halo=6, shrink=True, max_size=None, fixed=None,
              max_window=16384, frame_batch_size=10000, num_workers=0, device=None, ctx=None):
    """New supports and footprint values for the ROIs of ``demixed`` (a Demixed of ``pmd``) from the movie of ``kind``:
    "denoised" (of ``mean_img + var_img * (U R diag(s) Vt)``, the default; reads no movie) or "raw" (of ``movie``, in its
    own dtype, one read).  Returns a Grown.  With A = ``demixed.footprints`` (K x D, C pixel order) and C =
    ``demixed.traces``:

    1. the support of ROI k is {p : A[k, p] > 0}; its window the bounding box of the support widened by ``halo`` pixels
       on every side and clipped to the image.
    2. an ROI is fixed when ``fixed`` (row indices or a boolean (K,)) names it, ``demixed.empty`` marks it, or its
       window has more than ``max_window`` pixels (a full-field neuropil mask).  A fixed ROI keeps its support and
       values and is still taken out of the pixels of the others; an ROI without support is "empty" and has no row in
       ``rois``.
    3. for every pixel p of the window of a non-fixed ROI k, per frame in fp32: y = x_p, then for the other ROIs l with
       A[l, p] != 0 in ascending l: y = fl32(y - fl32(A[l, p] C[l, t])); the fp64 sums of y, y^2 and y C[k, t] over the
       frames, each one chain in ascending frame order with exact products.
    4. rho and beta = cov / var_c in float64 on the host (finish_moments): a variance at or below 3 (T + 2) 2^-53 T S2
       counts as zero and gives rho = 0.
    5. candidates are the window pixels with a finite rho > ``corr_th``; their 8-connected components that hold a pixel
       of the support are kept; the new support is their union (``shrink=False``: and the old support).  Nothing kept:
       the ROI stays as it is, status "lost".  With ``max_size`` and more pixels than that, the threshold goes up in
       steps of 0.1 while it stays below 1, then the ROI stays as it is, status "oversize" (grow_support).
    6. the new values are float32(beta); a pixel kept only through ``shrink=False`` with beta <= 0 keeps its value.

    ``Grown.rois`` numbers pixels in C order, like ``Demixed.footprints``: on a decomposition of order "C" it is a valid
    ``rois`` for demix and extract_traces as it is, on one of order "F" through ``in_pixel_order``.

    ``movie`` (of ``pmd.shape``; not needed, and never touched, for "denoised"): the sources of summary_images, read in
    ``frame_batch_size`` batches.  After ``pmd.to_device()`` its context and uploaded factors are reused.  Every result
    has the same bits for every frame_batch_size, source and residency, and for order "C" and "F" of the same movie.
    Argument errors are raised before any device work and before the movie is read; a decomposition of no frames raises
    ValueError, and so does a plan that does not fit the free device memory."""
    check_pmd(pmd)
    corr_th, halo, shrink, max_size, max_window = _check_grow(kind, corr_th, halo, shrink, max_size, max_window)
    T, d1, d2 = (int(x) for x in pmd.shape)
    D = d1 * d2
    if T == 0:
        raise ValueError("the decomposition has no frames: their correlations do not exist")
    if D >= 2 ** 31:
        raise ValueError("grow_rois numbers pixels in int32: {} pixels are too many".format(D))
    A, C = _check_demixed(demixed, T, D)
    K = A.shape[0]
    raw = kind == "raw"
    if raw and movie is None:
        raise ValueError('kind "raw" needs the movie: pass movie=')
    S = supports(A)
    win = windows(S, d1, d2, halo)
    status = roi_status(S, win, fixed_mask(K, fixed) | np.asarray(demixed.empty, dtype=bool), max_window)
    tabs = pair_tables(A, win, status == "grown", d2)
    n_pairs = len(tabs["pair_px"])
    kp = KindPlan(pmd, movie if raw else None, raw=raw, panels=() if raw else ("denoised",),
                  frame_batch_size=frame_batch_size)

    mom = np.zeros((3, 0))
    if n_pairs:
        with device_context(pmd, device, ctx) as (ctx, dv):
            nbytes = grow_device_bytes(**kp.facts(dv), kind=kind, K=K, n_pairs=n_pairs, n_others=len(tabs["oth_k"]))
            check_fit("grow_rois", nbytes, _device_free_bytes(ctx.device))
            mom = _window_moments(ctx, KindBlocks(ctx, pmd, dv, kp, num_workers), tabs, C)
    Sc, Scc = trace_sums(C)
    rho, beta = finish_moments(mom, T, Sc[tabs["pair_k"]], Scc[tabs["pair_k"]])
    rows, threshold, added, removed, status = grow_all(A, tabs, win, status, rho, beta, d2, corr_th, shrink, max_size)

    source = np.array([k for k in range(K) if status[k] != "empty"], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum([rows[k][0].size for k in source])]).astype(np.int64)
    rois = scipy.sparse.csr_matrix((np.concatenate([rows[k][1] for k in source]).astype(np.float32),
                                    np.concatenate([rows[k][0] for k in source]), indptr), shape=(len(source), D)) \
        if len(source) else scipy.sparse.csr_matrix((0, D), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        correlation = scipy.sparse.csr_matrix((rho.astype(np.float32), tabs["pair_px"].astype(np.int64), tabs["roi_ptr"]),
                                              shape=(K, D))
    return Grown(rois, source, np.asarray(demixed.labels)[source], correlation, threshold, added, removed, status)


def _window_moments(ctx, blocks, tabs, traces):
    """(3, n_pairs) float64: the sums of pmd_roi_window_moments_accumulate over the whole movie, block by block."""
    import torch
    from ._lib import ptr

    D = blocks.plan.D
    K = traces.shape[0]
    n_pairs = len(tabs["pair_px"])
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(ctx.device)   # noqa: E731
    pair_px, pair_k, oth_ptr = up(tabs["pair_px"]), up(tabs["pair_k"]), up(tabs["oth_ptr"])
    n_oth = len(tabs["oth_k"])
    oth_k = up(tabs["oth_k"] if n_oth else np.zeros(1, np.int32))
    oth_a = up(tabs["oth_a"] if n_oth else np.zeros(1, np.float32))
    ct = torch.empty((BLOCK, K), dtype=torch.float32, device=ctx.device)
    mom = torch.zeros((3, n_pairs), dtype=torch.float64, device=ctx.device)

    def before(c0, m, yp, elem):                              # the host waits here: ahead of the block's expansion
        ct[:m].copy_(torch.from_numpy(np.ascontiguousarray(traces[:, c0:c0 + m].T)))

    def each(c0, m, yp, elem, xp):
        X, e = (xp, 0) if xp is not None else (yp, elem)
        ctx.call("pmd_roi_window_moments_accumulate", X, int(e), D, D, int(m), ptr(ct), K, K, n_pairs, ptr(pair_px),
                 ptr(pair_k), ptr(oth_ptr), ptr(oth_k), ptr(oth_a), ptr(mom))

    blocks.run(each, before=before)
    ctx.sync()
    return mom.cpu().numpy()


def merge_rois(rois, traces, *, labels=None, corr_th=0.8, overlap_th=0.6, fixed=None):
    """Join ROIs that share most of their support and have correlated traces.  ``rois``: a sparse or dense (K, D) matrix
    of non-negative values, the supports S_k = {p : rois[k, p] > 0}; ``traces`` (K, T).  ROIs k and l are joined when
    |S_k & S_l| / min(|S_k|, |S_l|) > ``overlap_th`` and the float64 Pearson correlation of their traces is >
    ``corr_th`` (a constant trace correlates with nothing); only pairs that overlap are looked at, and an ROI of
    ``fixed`` (row indices or a boolean (K,)) joins nothing.  The groups are the connected components of that graph.  A
    group of several becomes the row sum_k rois[k] ||traces[k] - mean||_2 (float64, rounded to float32 once) with the
    label of its lowest member; a single ROI passes through with its bits.  Output rows are in ascending order of their
    lowest member.  Returns a Merged; ``labels`` defaults to the row numbers.  No device work."""
    if not _number(corr_th) or not -1.0 <= corr_th < 1.0:
        raise ValueError("corr_th must lie in [-1, 1), got {!r}".format(corr_th))
    if not _number(overlap_th) or not 0.0 <= overlap_th < 1.0:
        raise ValueError("overlap_th must lie in [0, 1), got {!r}".format(overlap_th))
    if not scipy.sparse.issparse(rois) and np.asarray(rois).ndim != 2:
        raise ValueError("rois must be a sparse or dense (K, D) matrix, got shape {}".format(np.asarray(rois).shape))
    R = scipy.sparse.csr_matrix(rois)
    if R.dtype.kind not in "biuf":
        raise ValueError("rois must be boolean or real numbers, got {}".format(R.dtype))
    R = R.astype(np.float32)
    R.sort_indices()
    K = R.shape[0]
    if R.nnz and (not np.all(np.isfinite(R.data)) or np.any(R.data < 0)):
        raise ValueError("rois hold negative or non-finite values")
    C = np.asarray(traces)
    if C.ndim != 2 or C.shape[0] != K or C.dtype.kind not in "iuf":
        raise ValueError("traces must be a numeric (K, T) array with K = {}, got {} {}".format(K, C.dtype, C.shape))
    labels = np.arange(K, dtype=np.int64) if labels is None else np.asarray(labels)
    if labels.shape != (K,):
        raise ValueError("labels must have shape ({},), got {}".format(K, labels.shape))
    free = ~fixed_mask(K, fixed)

    S = supports(R).astype(np.int64)
    size = np.asarray(S.sum(axis=1)).reshape(-1)
    both = scipy.sparse.triu(scipy.sparse.coo_matrix(S @ S.T), k=1).tocoo()
    C64 = C.astype(np.float64)
    dev = C64 - C64.mean(axis=1, keepdims=True) if C64.shape[1] else C64
    norm = np.sqrt((dev * dev).sum(axis=1))
    ek, el = [], []
    for k, l, n in zip(both.row, both.col, both.data):
        if n == 0 or not (free[k] and free[l]) or not n / min(size[k], size[l]) > overlap_th:
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.float64(dev[k] @ dev[l]) / (norm[k] * norm[l])
        if r > corr_th:                                       # a NaN compares false
            ek.append(k)
            el.append(l)
    graph = scipy.sparse.csr_matrix((np.ones(len(ek)), (ek, el)), shape=(K, K))
    n_groups, comp = scipy.sparse.csgraph.connected_components(graph, directed=False)
    groups = sorted((np.nonzero(comp == c)[0].astype(np.int64) for c in range(n_groups)), key=lambda g: int(g[0]))
    rows = []
    for g in groups:
        if len(g) == 1:
            rows.append(R[int(g[0])])
            continue
        acc = np.zeros(R.shape[1])
        for k in g:                                           # members in ascending order, one float64 sum per pixel
            s, e = R.indptr[k], R.indptr[k + 1]
            acc[R.indices[s:e]] += R.data[s:e].astype(np.float64) * norm[k]
        rows.append(scipy.sparse.csr_matrix(acc.astype(np.float32)[None, :]))
    out = scipy.sparse.vstack(rows, format="csr", dtype=np.float32) if rows else scipy.sparse.csr_matrix(R.shape, dtype=np.float32)
    out.sort_indices()
    return Merged(out, np.array([labels[int(g[0])] for g in groups], dtype=labels.dtype), groups)


def refine_demix(pmd, rois, movie=None, *, rounds=2, merge=True, grow_kw=None, merge_kw=None, **demix_kw):
    """``demix(pmd, rois, **demix_kw)``, then ``rounds`` times: ``grow_rois(pmd, demixed, movie, **grow_kw)``,
    ``merge_rois`` of the grown ROIs with the traces of their sources (``merge=False``: left out) and ``demix`` on the
    result.  A round that changes no support and merges nothing ends the loop before its demix.  Returns a Refined;
    ``rounds=0`` is demix.

    It is the composition of the three public calls and holds no state of its own.  What it carries from one round to the
    next: the labels (demix numbers the rows of a sparse ``rois`` anew, so the last Demixed gets the labels of the rows it
    was given), ``fixed`` of ``grow_kw`` (row indices or a boolean over the first round's ROIs; a row of a later round is
    fixed when one of the rows it came from was) and the ROIs grow_rois left fixed, which merge_rois does not join.
    ``device`` and ``ctx`` of ``demix_kw`` go to grow_rois as well."""
    from .demix import demix

    check_pmd(pmd)
    if not _is_int(rounds) or rounds < 0:
        raise ValueError("rounds must be an integer >= 0, got {!r}".format(rounds))
    grow_kw, merge_kw = dict(grow_kw or {}), dict(merge_kw or {})
    if "fixed" in merge_kw:
        raise ValueError("merge_kw may not hold fixed: it follows from grow_kw's fixed and the ROIs grow_rois leaves fixed")
    for key in ("device", "ctx"):
        if key in demix_kw:
            grow_kw.setdefault(key, demix_kw[key])
    fixed = grow_kw.pop("fixed", None)
    fov = tuple(int(x) for x in pmd.shape[1:])

    dm = demix(pmd, rois, **demix_kw)
    done = []
    fixed = fixed_mask(len(dm.labels), fixed) if rounds else None
    for _ in range(int(rounds)):
        g = grow_rois(pmd, dm, movie, fixed=fixed, **grow_kw)
        held = (g.status == "fixed")[g.source]
        m = merge_rois(g.rois, dm.traces[g.source], labels=g.labels, fixed=held, **merge_kw) if merge else None
        done.append((g, m))
        if not g.added.any() and not g.removed.any() and (m is None or len(m.groups) == g.rois.shape[0]):
            break
        new, labels = (m.rois, m.labels) if m is not None else (g.rois, g.labels)
        groups = m.groups if m is not None else [np.array([i]) for i in range(g.rois.shape[0])]
        fixed = np.array([bool(fixed[g.source[grp]].any()) for grp in groups], dtype=bool)
        dm = demix(pmd, in_pixel_order(new, fov, pmd.order), **demix_kw)
        dm.labels = np.asarray(labels)
    return Refined(dm, done)
