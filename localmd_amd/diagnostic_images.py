"""
Local correlation images of a movie and of its PMD approximation on the MI355X.

Same functions, arguments and results as the image routines of /root/reference/localmd/diagnostic_plots.py
(make_correlation_image :225-271, make_autocorrelation_image :274-304, make_pmd_correlation_image :166-223,
make_residual_correlation_image :100-163); the plotly figure builders of that file are not part of the hot path and
are not reproduced.  The reference loops over the pixels in Python and calls a jitted two-trace routine per neighbour
pair; here the frames stream through HBM once and two kernels (csrc/diag.hip) form every first and second moment, from
which all four images follow.  Movies: anything that slices like a (T, d1, d2) array - NumPy arrays, torch tensors (host
or device), a localmd_amd.PMDArray (expanded chunk by chunk).  Results: float64 (d1, d2) NumPy arrays, like the reference.

make_pmd_diagnostic_images(movie, pmd) computes all four images of a decomposition at once, plus the residual statistics,
reading the movie once in frame batches and reconstructing each batch on the device (csrc/diag_fused.hip).
"""
from typing import NamedTuple

import numpy as np

from ._lib import Context, ptr
from ._movie import _device_free_bytes, _stream_batch_frames
from ._stream import (batch_buffer_bytes, block_plan, check_fit, check_pmd, device_context, mean_std, read_batches,
                      scaled_r, source_info, upload_f32)

CHUNK_BYTES = 1 << 30


def _chunks(T, d1, d2, overlap=0):
    step = max(overlap + 1, CHUNK_BYTES // (4 * d1 * d2))
    t0 = 0
    while t0 < T:
        t1 = min(T, t0 + step)
        yield max(0, t0 - overlap), t0, t1
        t0 = t1


def _frames(movie, lo, hi, device):
    import torch

    x = movie[lo:hi]
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
    d1, d2 = (int(v) for v in movie.shape[1:])
    return x.to(device=device, dtype=torch.float32).reshape(hi - lo, d1, d2).contiguous()


def _neighbour_moments(ctx, movie, minus=None):
    """[10, D] float64 device tensor of the neighbour moments of movie (- minus)."""
    import torch

    T, d1, d2 = (int(v) for v in movie.shape)
    D = d1 * d2
    mom = torch.zeros((10, D), dtype=torch.float64, device=ctx.device)
    ref = None
    for lo, t0, t1 in _chunks(T, d1, d2):
        a = _frames(movie, t0, t1, ctx.device)
        b = _frames(minus, t0, t1, ctx.device) if minus is not None else None
        if ref is None:
            ref = (a[0] - b[0] if b is not None else a[0]).reshape(-1).clone()
        ws = ctx.workspace(ctx.lib.pmd_diag_workspace_bytes(t1 - t0, D))
        ctx.call("pmd_neighbour_moments", ptr(a), ptr(b), ptr(ref), t1 - t0, d1, d2, 1, ptr(mom), ptr(ws), ws.numel())
    return mom


def _image(ctx, num, den, T, d1, d2, kind, mode):
    import torch

    if mode not in ("max", "mean"):
        raise ValueError(f"mode {mode} not supported")
    out = torch.empty(d1 * d2, dtype=torch.float64, device=ctx.device)
    ctx.call("pmd_neighbour_image", ptr(num), ptr(den), T, d1, d2, kind, 0 if mode == "max" else 1, ptr(out))
    ctx.sync()
    return out.cpu().numpy().reshape(d1, d2)


def _with_ctx(fn):
    def wrapper(*args, device=None, ctx=None, **kw):
        own = ctx is None
        if own:
            ctx = Context(0 if device is None else device)
        try:
            return fn(ctx, *args, **kw)
        finally:
            if own:
                ctx.release_workspace()
                ctx.close()
    wrapper.__doc__ = fn.__doc__
    wrapper.__name__ = fn.__name__
    return wrapper


@_with_ctx
def make_correlation_image(ctx, movie, mode: str = "max"):
    """Pixel i = max (from 0) or mean over the adjacent pixels j of corr(movie_i, movie_j)  (diagnostic_plots.py:225-271)."""
    T, d1, d2 = (int(v) for v in movie.shape)
    mom = _neighbour_moments(ctx, movie)
    return _image(ctx, mom, None, T, d1, d2, 0, mode)


@_with_ctx
def make_pmd_correlation_image(ctx, original_movie, pmd_movie, mode: str = "max"):
    """Pixel i = Cov(pmd_i, pmd_j) / sqrt(Var(original_i) Var(original_j)), max / mean over the adjacent j
    (diagnostic_plots.py:166-223; jnp.cov has ddof 1, jnp.var ddof 0)."""
    T, d1, d2 = (int(v) for v in original_movie.shape)
    den = _neighbour_moments(ctx, original_movie)
    num = _neighbour_moments(ctx, pmd_movie)
    return _image(ctx, num, den, T, d1, d2, 1, mode)


@_with_ctx
def make_residual_correlation_image(ctx, original_movie, pmd_movie, mode: str = "max"):
    """Pixel i = Cov(original_i - pmd_i, original_j - pmd_j) / sqrt(Var(original_i) Var(original_j))
    (diagnostic_plots.py:100-163)."""
    T, d1, d2 = (int(v) for v in original_movie.shape)
    den = _neighbour_moments(ctx, original_movie)
    num = _neighbour_moments(ctx, original_movie, minus=pmd_movie)
    return _image(ctx, num, den, T, d1, d2, 1, mode)


@_with_ctx
def make_autocorrelation_image(ctx, movie, lag: int = 1):
    """Pixel i = corr(movie_i[lag:], movie_i[:-lag])  (diagnostic_plots.py:274-304)."""
    import torch

    T, d1, d2 = (int(v) for v in movie.shape)
    lag = int(lag)
    if lag < 1 or lag >= T:
        raise ValueError("lag must be in [1, frames)")
    D = d1 * d2
    mom = torch.zeros((5, D), dtype=torch.float64, device=ctx.device)
    ref = None
    for lo, t0, t1 in _chunks(T, d1, d2, overlap=lag):
        if t1 - lo <= lag:
            continue
        a = _frames(movie, lo, t1, ctx.device)
        if ref is None:
            ref = a[0].reshape(-1).clone()
        if lo > t0 - lag:       # first chunk: it has no `lag` frames in front of it, its pairs start at t = lag
            assert lo == 0
        ws = ctx.workspace(ctx.lib.pmd_diag_workspace_bytes(t1 - lo, D))
        ctx.call("pmd_lag_moments", ptr(a), ptr(ref), t1 - lo, D, lag, 1, ptr(mom), ptr(ws), ws.numel())
    out = torch.empty(D, dtype=torch.float64, device=ctx.device)
    ctx.call("pmd_lag_image", ptr(mom), D, T - lag, ptr(out))
    ctx.sync()
    return out.cpu().numpy().reshape(d1, d2)


# ---- one-pass diagnostics of a decomposition against its movie ------------------------------------------------------
DIAG_RECON_FRAMES = 2048    # frames per reconstruction block: bounds (R s) Vt, U (R s) Vt and its frames-first copy
DIAG_FRAME_BLOCK = 512      # frames per fp64 partial of pmd_diag_fused_accumulate: blocks start on multiples of it
DIAG_MOMENTS = 35           # 10 raw + 10 reconstruction + 10 residual neighbour moments, 5 raw lag moments


class PMDDiagnostics(NamedTuple):
    """Result of make_pmd_diagnostic_images.  The first four fields are in the argument order of the reference's
    make_pmd_corr_diagnostic_plot (diagnostic_plots.py), so ``make_pmd_corr_diagnostic_plot(*d[:4])`` works."""
    correlation: np.ndarray             # (d1, d2) make_correlation_image(movie, mode)
    autocorrelation: np.ndarray         # (d1, d2) make_autocorrelation_image(movie, lag)
    pmd_correlation: np.ndarray         # (d1, d2) make_pmd_correlation_image(movie, pmd_movie, mode)
    residual_correlation: np.ndarray    # (d1, d2) make_residual_correlation_image(movie, pmd_movie, mode)
    residual_std: np.ndarray            # (d1, d2) std over time (ddof 0) of movie - pmd_movie
    explained_variance: np.ndarray      # (d1, d2) 1 - var(movie - pmd_movie) / var(movie); NaN where var(movie) = 0
    frame_residual_rms: np.ndarray      # (T,) sqrt(mean over the pixels of (movie_t - pmd_movie_t)^2)


def diag_plan(T, frame_batch_size):
    """[(b0, b1, [(c0, c1), ...])]: the frame batches the movie is read in (those of the streamed decomposition, whole
    1024-frame chunks) and the reconstruction blocks of each, at most DIAG_RECON_FRAMES frames, starting on multiples of
    DIAG_FRAME_BLOCK."""
    return block_plan(T, frame_batch_size, min(_stream_batch_frames(frame_batch_size), DIAG_RECON_FRAMES))


def _fused_workspace_bytes(n, D):
    """pmd_diag_fused_workspace_bytes: the fp64 partials of the frame blocks and the per-frame residual sums."""
    blocks = -(-int(n) // DIAG_FRAME_BLOCK)
    return blocks * DIAG_MOMENTS * D * 8 + (-(-int(D) // 256)) * int(n) * 8


def _diag_device_bytes(D, nb, esize, n_cols, rank, nnz, lag, n_batches, host_source, factors_on_device):
    """(bytes, ring bytes) of device memory make_pmd_diagnostic_images holds for a movie of D pixels read in batches of
    nb frames, besides the T doubles of frame_residual_rms: no term grows with the movie's length.  Batch buffers (two
    for a host source, a converted copy at most for a device tensor), the Vt columns of one batch, one reconstruction
    block ((R s) Vt, U (R s) Vt and its frames-first copy), the kernel workspace, the moments and the per-pixel
    vectors, U and R s unless the PMDArray already holds them on the device, and the ring of `lag` raw frames for the
    lag pairs that cross a batch boundary."""
    rb = min(nb, DIAG_RECON_FRAMES)
    ldc = (rb + 3) // 4 * 4
    need = batch_buffer_bytes(nb, D, esize, host_source, n_batches)
    need += 4 * (n_cols * ldc + D * ldc + rb * D)
    need += _fused_workspace_bytes(rb, D) + DIAG_MOMENTS * D * 8 + 4 * D * 8 + (3 + 2 + 1) * D * 4
    if not factors_on_device:
        need += 4 * rank * nb + 8 * (D + 1) + 8 * nnz + 4 * n_cols * rank
    ring = lag * D * esize if n_batches > 1 else 0
    return need + ring, ring


def _check_fit(need, ring, free, lag):
    """ValueError before any allocation when the plan cannot fit; it names `lag` when the lag ring is what does not."""
    if need <= free:
        return
    if need - ring <= free:
        raise ValueError("make_pmd_diagnostic_images: the ring of lag = {} raw frames needs {:.2f} GB of device memory and "
                         "does not fit ({:.2f} GB free besides the batches); use a smaller lag".format(lag, ring / 1e9,
                                                                                                    (free - need + ring) / 1e9))
    check_fit("make_pmd_diagnostic_images", need, free)


def _check_args(original_movie, pmd, mode, lag):
    check_pmd(pmd)
    shape = tuple(int(x) for x in pmd.shape)
    on_device, esize = source_info(original_movie, shape)
    if mode not in ("max", "mean"):
        raise ValueError(f"mode {mode} not supported")
    if isinstance(lag, bool) or int(lag) != lag:
        raise ValueError("lag must be an integer, got {!r}".format(lag))
    lag = int(lag)
    if lag < 1 or lag >= shape[0]:
        raise ValueError("lag must be in [1, frames): lag = {}, {} frames".format(lag, shape[0]))
    return shape, lag, on_device, esize


def make_pmd_diagnostic_images(original_movie, pmd, *, mode="max", lag=1, frame_batch_size=10000, num_workers=0,
                               device=None, ctx=None):
    """All four diagnostic images of a decomposition (make_correlation_image, make_autocorrelation_image,
    make_pmd_correlation_image and make_residual_correlation_image with pmd_movie = pmd[:]) plus the residual
    statistics, from ONE read of ``original_movie``.  Returns a PMDDiagnostics.

    ``pmd`` is a PMDArray; after ``pmd.to_device()`` its context and uploaded factors are reused.  Sources: NumPy arrays
    and memmaps, any lazy_data_loader (TiffArray included) and CPU tensors, read in ``frame_batch_size`` batches (rounded
    down to whole 1024-frame chunks) through the pinned staging ring of the streamed decomposition, uint16 / int16 in their
    own dtype; device tensors are sliced in place with the same batches.  Each batch is reconstructed on the device
    ((R s) Vt[:, batch] with pmd_gemm, then U and the noise image with the expansion kernels) and one fused kernel forms
    the moments of the movie, the reconstruction and the residual; device memory does not grow with the movie's length
    except for the T doubles of frame_residual_rms."""
    (T, d1, d2), lag, on_device, esize = _check_args(original_movie, pmd, mode, lag)
    D = d1 * d2
    plan = diag_plan(T, frame_batch_size)
    nb = plan[0][1] - plan[0][0]
    rb = min(nb, DIAG_RECON_FRAMES)
    ldc = (rb + 3) // 4 * 4
    n_cols, rank = (int(x) for x in pmd.r.shape)
    with device_context(pmd, device, ctx) as (ctx, dv):
        need, ring_bytes = _diag_device_bytes(D, nb, esize, n_cols, rank, int(pmd.u.nnz), lag, len(plan), not on_device,
                                              dv is not None)
        _check_fit(need + 8 * T, ring_bytes, _device_free_bytes(ctx.device), lag)
        return _diagnostics(ctx, original_movie, pmd, dv, plan, T, d1, d2, mode, lag, rb, ldc, n_cols, rank,
                            frame_batch_size, num_workers)


def _diagnostics(ctx, movie, pmd, dv, plan, T, d1, d2, mode, lag, rb, ldc, n_cols, rank, frame_batch_size, num_workers):
    import ctypes as C

    import torch
    dev = ctx.device
    D = d1 * d2
    mean, std = mean_std(ctx, pmd)
    # U row of C-order pixel c (the decomposition's pixel order), as PMDArray._getitem_device selects them
    sel = torch.from_numpy(np.ascontiguousarray(pmd.row_indices.reshape(-1), dtype=np.int32)).to(dev)
    if dv is not None:
        indptr, indices, data, vt_all = dv["indptr"], dv["indices"], dv["data"], dv["v"]
    else:
        u = pmd.u
        indptr = torch.from_numpy(u.indptr.astype(np.int64)).to(dev)
        indices = torch.from_numpy(u.indices.astype(np.int32)).to(dev)
        data = upload_f32(ctx, u.data)
        vt_all = None
    rs = scaled_r(ctx, pmd, dv)
    expand = rank > 0 and n_cols > 0
    ct = torch.zeros((n_cols, ldc), dtype=torch.float32, device=dev) if expand else None
    acc = torch.empty((D, ldc), dtype=torch.float32, device=dev) if expand else None
    W = torch.empty((rb, D), dtype=torch.float32, device=dev)
    ws = torch.empty(int(ctx.lib.pmd_diag_fused_workspace_bytes(rb, D)), dtype=torch.uint8, device=dev)
    mom = torch.zeros((DIAG_MOMENTS, D), dtype=torch.float64, device=dev)
    ref = torch.empty((3, D), dtype=torch.float32, device=dev)
    fss = torch.empty(T, dtype=torch.float64, device=dev)
    st = {"ring": None, "vt": None, "pin": [None, None], "ev": [None, None], "k": 0}
    last_b0 = plan[-1][0]
    blocks = {b0: cb for b0, _, cb in plan}

    def vt_batch(b0, n):
        """(device pointer of Vt[:, b0], leading dimension): the whole Vt of a to_device() PMDArray, else the batch's
        columns uploaded through two page-locked buffers."""
        if vt_all is not None:
            return vt_all[:, b0:].data_ptr(), T
        j = st["k"] % 2
        st["k"] += 1
        if st["pin"][j] is None or st["pin"][j].numel() < rank * n:
            st["pin"][j] = torch.empty(rank * n, dtype=torch.float32, pin_memory=True)
        elif st["ev"][j] is not None:
            st["ev"][j].synchronize()           # the upload that last read this buffer has finished
        np.copyto(st["pin"][j][:rank * n].numpy().reshape(rank, n), pmd.v[:, b0:b0 + n], casting="unsafe")
        if st["vt"] is None or st["vt"].numel() < rank * n:
            st["vt"] = torch.empty(rank * n, dtype=torch.float32, device=dev)
        st["vt"][:rank * n].copy_(st["pin"][j][:rank * n], non_blocking=True)
        st["ev"][j] = torch.cuda.Event()
        st["ev"][j].record(torch.cuda.current_stream(dev))
        return st["vt"].data_ptr(), n

    def consume(batch, elem, b0, n):
        esize = batch.element_size()
        if expand:
            vp, ldv = vt_batch(b0, n)
        for c0, c1 in blocks[b0]:
            m = c1 - c0
            if expand:
                m4 = min((m + 3) // 4 * 4, ldc)
                ctx.call("pmd_gemm", 0, 0, n_cols, m, rank, 1.0, ptr(rs), rank, C.c_void_p(vp + 4 * (c0 - b0)), ldv, 0.0,
                         ptr(ct), ldc)
                ctx.call("pmd_csr_rows_spmm", ptr(indptr), ptr(indices), ptr(data), ptr(sel), D, ptr(ct), ldc, m4, ptr(acc),
                         ldc)
                ctx.call("pmd_transpose_affine", ptr(acc), ldc, D, m, ptr(std), None, ptr(W), D)
            else:
                W[:m].zero_()
            ctx.call("pmd_diag_fused_accumulate", ptr(batch), int(elem), b0, ptr(W), ptr(st["ring"]), lag, c0, m, T, d1, d2,
                     ptr(mean), ptr(ref), ptr(mom), ptr(fss), ptr(ws), ws.numel())
        if b0 != last_b0:
            # the last `lag` frames read so far go to ring slot (frame mod lag) for the pairs of the next batches
            if st["ring"] is None:
                st["ring"] = torch.empty((lag, D), dtype=batch.dtype, device=dev)
            rb8, bb8 = st["ring"].view(torch.uint8), batch.reshape(n, D).view(torch.uint8)
            t = max(b0, b0 + n - lag)
            while t < b0 + n:
                s = t % lag
                k = min(b0 + n - t, lag - s)
                rb8[s:s + k].copy_(bb8[t - b0:t - b0 + k])
                t += k

    read_batches(ctx, movie, [(b0, b1) for b0, b1, _ in plan], frame_batch_size, num_workers, consume)

    img = torch.empty((4, D), dtype=torch.float64, device=dev)
    m_code = 0 if mode == "max" else 1
    ctx.call("pmd_neighbour_image", ptr(mom[0]), None, T, d1, d2, 0, m_code, ptr(img[0]))
    ctx.call("pmd_lag_image", ptr(mom[30]), D, T - lag, ptr(img[1]))
    ctx.call("pmd_neighbour_image", ptr(mom[10]), ptr(mom[0]), T, d1, d2, 1, m_code, ptr(img[2]))
    ctx.call("pmd_neighbour_image", ptr(mom[20]), ptr(mom[0]), T, d1, d2, 1, m_code, ptr(img[3]))
    # residual statistics from the shifted residual sums (shift invariant); the per-frame sums are unshifted
    var_y = ((mom[1] - mom[0] * mom[0] / T) / T).clamp_min(0.0)
    var_r = ((mom[21] - mom[20] * mom[20] / T) / T).clamp_min(0.0)
    ev = torch.where(var_y > 0, 1.0 - var_r / torch.where(var_y > 0, var_y, 1.0), torch.full_like(var_y, float("nan")))
    rms = torch.sqrt(fss / D)
    res = torch.stack([var_r.sqrt(), ev])
    ctx.sync()
    img, res, rms = img.cpu().numpy(), res.cpu().numpy(), rms.cpu().numpy()
    return PMDDiagnostics(*(img[k].reshape(d1, d2) for k in range(4)), res[0].reshape(d1, d2), res[1].reshape(d1, d2), rms)
