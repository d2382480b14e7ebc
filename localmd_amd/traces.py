"""
ROI traces of a decomposition: the time course of a set of weighted pixel masks, denoised, raw, and their difference.

``extract_traces(pmd, rois, movie, kinds=("denoised", "raw", "residual"))`` returns (K, T) float32 arrays for K masks
with weights ``W`` (K x D):

* denoised ``W x = W mean + (W diag(std) U) (R diag(s)) Vt`` never touches a pixel: ``B = W diag(std) U`` is built on the
  host with SciPy in float64 (a few hundred nonzeros per row, never the dense K x n_cols matrix), ``Wk = B (R diag(s))``
  is one ``pmd_csr_rows_spmm`` and every 1024-frame block one ``pmd_gemm`` ``Wk Vt[:, block]`` (blocks start on multiples
  of 1024 whatever the batch size, so every product has the same shape and every output bit is the same for every
  batching and source); ``pmd_roi_combine`` adds the offset ``W mean`` and forms the residual;
* raw ``W y`` reads the masked pixels of the movie once: ``pmd_roi_gather`` (csrc/roi.hip) on every frame batch in its
  source dtype, driven by the tables built here (roi_tables);
* residual is raw - denoised of the returned float32 values, element by element.

The movie is read once in the frame batches of the streamed decomposition (host sources through its pinned staging ring,
device tensors sliced in place); the traces leave the device batch by batch through the pinned ring of
``_stream.ToHost``.  Device memory does not grow with the movie's length.
"""
import numpy as np
import scipy.sparse

from ._movie import _device_free_bytes
from ._stream import (BLOCK, ToHost, VtBlocks, batch_buffer_bytes, block_plan, block_walk, check_fit, check_pmd,
                      device_context, factor_bytes, name_tuple, read_batches, scaled_r, source_info, upload_f32)

KINDS = ("denoised", "raw", "residual")
REDUCE = ("mean", "sum")
ROI_SEG = 1024        # pixels per segment: a longer ROI is cut into segments whose partial sums are added in order
ROI_CHUNK = 64        # pixels per step of a wave (one per lane)
SEG_FIELDS = 4        # {q0, p, out_row, to_ws}
SPLIT_FIELDS = 3      # {out_row, ws_row0, parts}


class Traces:
    """Result of extract_traces: ``denoised``, ``raw``, ``residual`` ((K, T) float32, or None when not asked for) and
    ``labels`` ((K,) the label of each row)."""

    def __init__(self, labels, denoised=None, raw=None, residual=None):
        self.labels, self.denoised, self.raw, self.residual = labels, denoised, raw, residual

    def __repr__(self):
        have = [k for k in KINDS if getattr(self, k) is not None]
        return "Traces({} ROIs, {})".format(len(self.labels), ", ".join(have))


# ---- argument checks and tables (no device work) --------------------------------------------------------------------
def roi_weights(rois, fov, order, reduce="sum"):
    """(W, labels): the K x D float64 CSR weight matrix of ``rois`` with columns numbering pixels in C order
    (c = i d2 + j), indices ascending within a row and explicit zeros dropped, and the (K,) int64 labels of its rows.

    ``rois``: a (K, d1, d2) boolean or numeric array; a (d1, d2) integer label image (0 = no ROI; one boolean mask per
    label, rows in ascending label order); or a scipy.sparse matrix (K, d1 d2) whose columns number pixels in ``order``
    (the way the rows of U do).  ``reduce="mean"`` divides every row by its sum."""
    d1, d2 = (int(x) for x in fov)
    D = d1 * d2
    if order not in ("C", "F"):
        raise ValueError("order must be 'C' or 'F', got {!r}".format(order))
    if reduce not in REDUCE:
        raise ValueError("unknown reduce {!r}; choose from {}".format(reduce, REDUCE))
    if scipy.sparse.issparse(rois):
        if rois.ndim != 2 or rois.shape[1] != D:
            raise ValueError("sparse rois have shape {}, the field of view {} x {} needs (K, {})".format(
                tuple(rois.shape), d1, d2, D))
        coo = scipy.sparse.coo_matrix(rois)
        if coo.dtype.kind not in "biuf":
            raise ValueError("rois must be boolean or real numbers, got {}".format(coo.dtype))
        # pixel id in `order` (a row of U) -> C-order pixel id
        c_of_u = np.empty(D, dtype=np.int64)
        c_of_u[np.arange(D).reshape((d1, d2), order=order).reshape(-1)] = np.arange(D)
        W = scipy.sparse.csr_matrix((coo.data.astype(np.float64), (coo.row, c_of_u[coo.col])), shape=coo.shape)
        labels = np.arange(W.shape[0], dtype=np.int64)
    else:
        a = np.asarray(rois)
        if a.dtype.kind not in "biuf":
            raise ValueError("rois must be boolean, integer or real numbers, got {}".format(a.dtype))
        if a.ndim == 3:
            if a.shape[1:] != (d1, d2):
                raise ValueError("rois have the field of view {} x {}, the decomposition {} x {}".format(
                    a.shape[1], a.shape[2], d1, d2))
            W = scipy.sparse.csr_matrix(a.reshape(a.shape[0], D)).astype(np.float64)
            labels = np.arange(a.shape[0], dtype=np.int64)
        elif a.ndim == 2:
            if a.shape != (d1, d2):
                raise ValueError("the label image has shape {}, the field of view is {} x {}".format(a.shape, d1, d2))
            if a.dtype.kind not in "iu":
                raise ValueError("a (d1, d2) label image must be integer, got {} (pass one mask as (1, d1, d2))".format(
                    a.dtype))
            if a.size and a.min() < 0:
                raise ValueError("the label image has negative labels")
            flat = a.reshape(-1)
            c = np.nonzero(flat)[0]
            labels, row = np.unique(flat[c], return_inverse=True)
            labels = labels.astype(np.int64)
            W = scipy.sparse.csr_matrix((np.ones(c.size), (row.reshape(-1), c)), shape=(len(labels), D))
        else:
            raise ValueError("rois must be shaped (K, d1, d2) or (d1, d2), or a sparse (K, d1 d2) matrix; got {}".format(
                a.shape))
    W.sum_duplicates()
    if not np.all(np.isfinite(W.data)):
        raise ValueError("rois hold non-finite weights")
    W.eliminate_zeros()
    W.sort_indices()
    K = W.shape[0]
    if K == 0:
        raise ValueError("rois hold no ROI (K = 0)")
    npx = np.diff(W.indptr)
    if np.any(npx == 0):
        raise ValueError("ROI {} has no pixels".format(int(labels[int(np.argmax(npx == 0))])))
    if reduce == "mean":
        tot = np.asarray(W.sum(axis=1)).reshape(-1)
        if np.any(~(tot > 0)):
            raise ValueError("reduce='mean': the weights of ROI {} sum to {} (<= 0)".format(
                int(labels[int(np.argmax(~(tot > 0)))]), float(tot[int(np.argmax(~(tot > 0)))])))
        W = scipy.sparse.csr_matrix((W.data / np.repeat(tot, npx), W.indices, W.indptr), shape=W.shape)
    w32 = W.data.astype(np.float32)
    if not np.all(np.isfinite(w32)) or np.any(w32 == 0):
        raise ValueError("rois hold weights outside the float32 range")
    return W, labels


def roi_tables(rois, fov, order, reduce="sum", seg=ROI_SEG):
    """The tables of pmd_roi_gather for ``rois`` (see roi_weights) on the field of view ``fov``, as NumPy arrays:

    ptr      int64 (K + 1,)   pixels of ROI k: ptr[k] .. ptr[k + 1]
    pix      int32            C-order pixel ids of all ROIs, ascending within an ROI
    w        float32          their weights (W rounded once)
    segs     int64 (S, 4)     {q0, p, out_row, to_ws}: p <= seg pixels from q0; a whole ROI (to_ws = 0, row out_row of
                              the output) or one piece of a split ROI (to_ws = 1, row out_row of the workspace)
    split    int64 (M, 3)     {out_row, ws_row0, parts} per split ROI: its pieces are workspace rows ws_row0 + c
    W, labels, K, D, n_partial_rows, seg
    """
    seg = int(seg)
    if seg < ROI_CHUNK or seg % ROI_CHUNK:
        raise ValueError("seg must be a positive multiple of {}".format(ROI_CHUNK))
    W, labels = roi_weights(rois, fov, order, reduce)
    K, D = W.shape
    ptr = W.indptr.astype(np.int64)
    npx = np.diff(ptr)
    parts = -(-npx // seg)
    n_seg = int(parts.sum())
    roi_of = np.repeat(np.arange(K, dtype=np.int64), parts)
    first = np.concatenate([[0], np.cumsum(parts)[:-1]])
    piece = np.arange(n_seg, dtype=np.int64) - np.repeat(first, parts)
    q0 = ptr[roi_of] + piece * seg
    p = np.minimum(seg, ptr[roi_of + 1] - q0)
    is_split = parts > 1
    ws_row0 = np.concatenate([[0], np.cumsum(np.where(is_split, parts, 0))[:-1]]).astype(np.int64)
    to_ws = is_split[roi_of].astype(np.int64)
    out_row = np.where(to_ws == 1, ws_row0[roi_of] + piece, roi_of)
    split_rois = np.nonzero(is_split)[0]
    tabs = {
        "ptr": ptr, "pix": W.indices.astype(np.int32), "w": W.data.astype(np.float32),
        "segs": np.stack([q0, p, out_row, to_ws], axis=1).astype(np.int64).reshape(-1, SEG_FIELDS),
        "split": np.stack([split_rois, ws_row0[split_rois], parts[split_rois]], axis=1).astype(np.int64).reshape(
            -1, SPLIT_FIELDS),
        "W": W, "labels": labels, "K": int(K), "D": int(D), "n_partial_rows": int(parts[is_split].sum()), "seg": seg,
    }
    validate_roi_tables(tabs)
    return tabs


def validate_roi_tables(t):
    """Raise ValueError unless every index pmd_roi_gather follows stays inside its array and every output row is written
    exactly once (the kernel trusts the tables)."""
    ptr, pix, w, segs, split = t["ptr"], t["pix"], t["w"], t["segs"], t["split"]
    K, D, n_ws, seg = int(t["K"]), int(t["D"]), int(t["n_partial_rows"]), int(t["seg"])
    if (ptr.shape != (K + 1,) or segs.ndim != 2 or segs.shape[1] != SEG_FIELDS or split.ndim != 2
            or split.shape[1] != SPLIT_FIELDS or pix.ndim != 1 or w.shape != pix.shape or K < 1):
        raise ValueError("roi tables: bad table shapes")
    if ptr[0] != 0 or ptr[-1] != pix.size or np.any(np.diff(ptr) < 1):
        raise ValueError("roi tables: pixel offsets are not increasing / do not cover the pixel list")
    if int(pix.min()) < 0 or int(pix.max()) >= D:
        raise ValueError("roi tables: pixel id outside [0, {})".format(D))
    inner = np.ones(pix.size, dtype=bool)
    inner[ptr[:-1]] = False
    if np.any((np.diff(pix.astype(np.int64), prepend=-1) <= 0) & inner):
        raise ValueError("roi tables: the pixel ids of an ROI are not ascending")
    if not np.all(np.isfinite(w)):
        raise ValueError("roi tables: non-finite weight")
    q0, p, out_row, to_ws = (segs[:, k] for k in range(SEG_FIELDS))
    if np.any(p < 1) or np.any(p > seg) or not np.all((to_ws == 0) | (to_ws == 1)):
        raise ValueError("roi tables: a segment has a pixel count outside [1, {}] or a bad flag".format(seg))
    if len(segs) == 0 or q0[0] != 0 or np.any(q0[1:] != q0[:-1] + p[:-1]) or q0[-1] + p[-1] != pix.size:
        raise ValueError("roi tables: the segments do not cover the pixel list once, in order")
    roi_of = np.searchsorted(ptr, q0, side="right") - 1
    if np.any(q0 + p > ptr[roi_of + 1]):
        raise ValueError("roi tables: a segment crosses into the next ROI")
    sp_out, sp_row0, sp_parts = (split[:, k] for k in range(SPLIT_FIELDS))
    if np.any(sp_parts < 2) or np.any(sp_out < 0) or np.any(sp_out >= K) or len(np.unique(sp_out)) != len(sp_out):
        raise ValueError("roi tables: a split entry names a bad output row or fewer than two parts")
    if int(sp_parts.sum()) != n_ws or np.any(sp_row0 != np.concatenate([[0], np.cumsum(sp_parts)[:-1]])):
        raise ValueError("roi tables: the split entries do not cover the partial-sum workspace once, in order")
    direct = to_ws == 0
    if np.any(out_row[direct] != roi_of[direct]) or np.any(np.isin(roi_of[direct], sp_out)):
        raise ValueError("roi tables: a whole-ROI segment writes another ROI's row")
    rows_written = np.sort(np.concatenate([out_row[direct], sp_out]))
    if not np.array_equal(rows_written, np.arange(K)):
        raise ValueError("roi tables: the output rows are not written exactly once")
    if np.any(~direct):
        ws_rows, ws_roi = out_row[~direct], roi_of[~direct]
        if not np.array_equal(ws_rows, np.arange(n_ws)):
            raise ValueError("roi tables: the workspace rows are not written exactly once, in order")
        owner = np.repeat(sp_out, sp_parts)
        if not np.array_equal(owner, ws_roi):
            raise ValueError("roi tables: a workspace row belongs to another ROI than its split entry")
    elif n_ws:
        raise ValueError("roi tables: partial rows without split segments")


def denoised_factors(pmd, W):
    """(B, offset): ``B = W diag(std) U`` (K x n_cols CSR, float64, computed sparse) and ``offset = W mean`` (K,) float64
    for the C-order weight matrix ``W`` of roi_weights.  The few columns of W are scaled by the std image and moved into
    U's row order (pmd.order), so U itself is used as stored (pmd.var_img is the std image, stored under the reference's
    name)."""
    u_of_c = np.asarray(pmd.row_indices).reshape(-1)             # row of U that holds C-order pixel c
    std = np.asarray(pmd.var_img, dtype=np.float64).reshape(-1)
    mean = np.asarray(pmd.mean_img, dtype=np.float64).reshape(-1)
    coo = W.tocoo()
    w_u = scipy.sparse.csr_matrix((coo.data.astype(np.float64) * std[coo.col], (coo.row, u_of_c[coo.col])), shape=W.shape)
    B = scipy.sparse.csr_matrix(w_u @ pmd.u, dtype=np.float64)
    B.sort_indices()
    return B, np.asarray(W @ mean, dtype=np.float64).reshape(-1)


def traces_device_bytes(D, nb, esize, K, n_out, n_scratch, nnz_w, n_segs, n_split, n_partial_rows, nnz_b, n_cols, rank,
                        needs_movie, host_source, n_batches, factors_on_device):
    """Device bytes extract_traces holds for K masks on a movie of D pixels read in batches of nb frames; no term grows
    with the movie's length.  Batch buffers (two for a host source, a converted copy at most for a device tensor), the
    output ring (two buffers of n_out K x nb traces), n_scratch K x nb scratch rows (raw traces that are needed but not
    returned), the partial sums of split ROIs, one block of Vt columns and of Wk Vt, Wk, B, the tables, and R s unless
    the PMDArray already holds it on the device."""
    need = 0
    if needs_movie:
        need += batch_buffer_bytes(nb, D, esize, host_source, n_batches)
        need += 8 * nnz_w + 8 * (SEG_FIELDS * n_segs + SPLIT_FIELDS * n_split) + 4 * n_partial_rows * nb
    need += 4 * K * nb * (2 * n_out + n_scratch)
    need += 4 * (K * BLOCK + K * rank + K) + 12 * nnz_b + 8 * (K + 1)
    need += factor_bytes(n_cols, rank, factors_on_device)
    return need + (1 << 20)     # the allocator's rounding of the small arrays


def _check_fit(need, free):
    check_fit("extract_traces", need, free)


# ---- public entry point --------------------------------------------------------------------------------------------
def extract_traces(pmd, rois, movie=None, *, kinds=("denoised",), reduce="mean", frame_batch_size=10000, num_workers=0,
                   device=None, ctx=None):
    """Traces of the masks ``rois`` (see roi_weights for the three forms): ``kinds`` is any non-empty subset of
    "denoised" (W applied to ``mean_img + var_img * (U R diag(s) Vt)``; no movie is read), "raw" (W applied to
    ``movie``) and "residual" (raw - denoised of the returned values).  ``reduce="mean"`` gives weighted averages (each
    mask's weights are divided by their sum), ``"sum"`` uses the weights as given.  Returns a Traces object with (K, T)
    float32 arrays (None for kinds not asked for) and ``labels``.

    ``movie`` (needed by "raw" and "residual", of ``pmd.shape``): NumPy arrays and memmaps, any lazy_data_loader
    (TiffArray included), CPU tensors (read once in ``frame_batch_size`` batches through the pinned staging ring of the
    streamed decomposition, uint16 / int16 in their own dtype) and device tensors (sliced in place).  After
    ``pmd.to_device()`` its context and uploaded factors are reused.  Every trace has the same bits for every
    frame_batch_size and source.  Argument errors are raised before any device work and before the movie is read."""
    check_pmd(pmd)
    kinds = name_tuple(kinds, KINDS, "kind", "kinds")
    if reduce not in REDUCE:
        raise ValueError("unknown reduce {!r}; choose from {}".format(reduce, REDUCE))
    T, d1, d2 = (int(x) for x in pmd.shape)
    D = d1 * d2
    needs_movie = any(k != "denoised" for k in kinds)
    needs_den = any(k != "raw" for k in kinds)
    if needs_movie and movie is None:
        raise ValueError("kinds {} need the movie: pass movie=".format(tuple(k for k in kinds if k != "denoised")))
    on_device, esize = source_info(movie, pmd.shape) if movie is not None else (False, 4)
    tabs = roi_tables(rois, (d1, d2), pmd.order, reduce)
    K = tabs["K"]
    n_cols, rank = (int(x) for x in pmd.r.shape)
    B = offset = None
    if needs_den:
        B, offset = denoised_factors(pmd, tabs["W"])
        if B.shape != (K, n_cols):
            raise ValueError("U has {} columns, R has {} rows".format(B.shape[1], n_cols))
    plan = block_plan(T, frame_batch_size)
    if not plan:        # a movie without frames
        return Traces(tabs["labels"], **{k: np.zeros((K, 0), dtype=np.float32) for k in kinds})
    nb = plan[0][1] - plan[0][0]

    with device_context(pmd, device, ctx) as (ctx, dv):
        n_scratch = 1 if "residual" in kinds and "raw" not in kinds else 0
        need = traces_device_bytes(D, nb, esize, K, len(kinds), n_scratch, tabs["pix"].size, len(tabs["segs"]),
                                   len(tabs["split"]), tabs["n_partial_rows"], B.nnz if B is not None else 0, n_cols, rank,
                                   needs_movie, not on_device, len(plan), dv is not None)
        _check_fit(need, _device_free_bytes(ctx.device))
        out = _extract(ctx, pmd, dv, tabs, B, offset, movie if needs_movie else None, plan, kinds, frame_batch_size,
                       num_workers)
    return Traces(tabs["labels"], **out)


class DeviceRoiTables:
    """The ROI tables on the device, ready for pmd_roi_gather."""

    def __init__(self, ctx, tabs):
        import torch

        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)   # noqa: E731
        self.ctx = ctx
        self.D, self.K = int(tabs["D"]), int(tabs["K"])
        self.n_segs, self.n_split = len(tabs["segs"]), len(tabs["split"])
        self.n_partial_rows = int(tabs["n_partial_rows"])
        self.segs = up(tabs["segs"].reshape(-1))
        self.split = up(tabs["split"].reshape(-1)) if self.n_split else None
        self.pix, self.w = up(tabs["pix"]), up(tabs["w"])

    def workspace_bytes(self, n):
        return int(self.ctx.lib.pmd_roi_gather_workspace_bytes(self.n_partial_rows, int(n)))

    def gather(self, batch, elem, n, out, ldo, ws):
        """out[:K, :n] (ld ldo) = W applied to the frames-first batch (n x D, element type elem)."""
        from ._lib import ptr

        self.ctx.call("pmd_roi_gather", ptr(batch), int(elem), int(n), self.D, self.n_segs, ptr(self.segs), ptr(self.pix),
                      ptr(self.w), self.n_partial_rows, self.n_split, ptr(self.split), ptr(out), int(ldo), ptr(ws),
                      0 if ws is None else ws.numel())


def _extract(ctx, pmd, dv, tabs, B, offset, movie, plan, kinds, frame_batch_size, num_workers):
    import torch
    from ._lib import ptr

    T = int(pmd.shape[0])
    dev = ctx.device
    K = tabs["K"]
    n_cols, rank = (int(x) for x in pmd.r.shape)
    BL = BLOCK
    nb = plan[0][1] - plan[0][0]
    needs_den = B is not None
    product = needs_den and rank > 0 and n_cols > 0
    rt = DeviceRoiTables(ctx, tabs) if movie is not None else None
    ws_bytes = rt.workspace_bytes(nb) if rt is not None else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    if needs_den:
        off_dev = upload_f32(ctx, offset)
    if product:
        rs = scaled_r(ctx, pmd, dv)
        wk = torch.empty((K, rank), dtype=torch.float32, device=dev)
        b_ptr = torch.from_numpy(B.indptr.astype(np.int64)).to(dev)
        b_idx = torch.from_numpy(B.indices.astype(np.int32) if B.nnz else np.zeros(1, np.int32)).to(dev)
        b_val = upload_f32(ctx, B.data if B.nnz else np.zeros(1))
        ctx.call("pmd_csr_rows_spmm", ptr(b_ptr), ptr(b_idx), ptr(b_val), None, K, ptr(rs), rank, rank, ptr(wk), rank)
        vt = VtBlocks(ctx, pmd, dv)
        ct = torch.empty((K, BL), dtype=torch.float32, device=dev)
    sink = ToHost(ctx, len(kinds) * K, T)
    scratch = (torch.empty(K * nb, dtype=torch.float32, device=dev)
               if "residual" in kinds and "raw" not in kinds else None)
    F = 4   # bytes per output value
    walk = block_walk(plan, tabs["D"])

    def consume(batch, elem, b0, n):
        buf, ld = sink.dst(b0, n)
        row = {k: buf.data_ptr() + F * j * K * ld for j, k in enumerate(kinds)}      # K x n panels, ld n
        raw_p = row.get("raw", scratch.data_ptr() if scratch is not None else None)
        if batch is not None:
            rt.gather(batch, elem, n, _Ptr(raw_p), ld, ws)
        if needs_den:
            den_p, res_p = row.get("denoised"), row.get("residual")
            for c0, m, _ in walk(None, b0):      # the traces are addressed in the output buffer, not in the batch
                o = F * (c0 - b0)
                if product:
                    vt.load(c0, m)
                    ctx.call("pmd_gemm", 0, 0, K, m, rank, 1.0, ptr(wk), rank, ptr(vt.buf), BL, 0.0, ptr(ct), BL)
                ctx.call("pmd_roi_combine", K, m, ptr(ct) if product else None, BL, ptr(off_dev),
                         _cp(raw_p, o) if res_p is not None else None, ld, _cp(den_p, o), ld, _cp(res_p, o), ld)
        sink.done(b0, n)

    read_batches(ctx, movie, [(b0, b1) for b0, b1, _ in plan], frame_batch_size, num_workers, consume)
    sink.finish()
    ctx.sync()
    return {k: np.ascontiguousarray(sink.out[j * K:(j + 1) * K]) for j, k in enumerate(kinds)}


class _Ptr:
    """A raw device address with the data_ptr() of a tensor (for _lib.ptr)."""

    def __init__(self, address):
        self.address = int(address)

    def data_ptr(self):
        return self.address


def _cp(base, offset):
    """c_void_p of base + offset bytes; None stays NULL."""
    import ctypes as C

    return None if base is None else C.c_void_p(int(base) + int(offset))
