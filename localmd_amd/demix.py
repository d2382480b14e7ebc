"""
Demixing of overlapping ROIs: non-negative footprints and traces fitted to the denoised movie in the compressed domain.

``demix(pmd, rois)`` minimises ``|| X - A C - b 1^T ||_F^2`` over footprints ``A >= 0`` (D x K, column k non-zero only on
the pixels of ROI k, its support, fixed for the whole call; a full-field mask acts as a neuropil component), traces
``C`` (K x T, rows >= 0 unless ``nonneg_traces=False``) and a free static background image ``b``, where
``X = mean 1^T + Uh Q V`` is the denoised movie (``Uh = diag(std) U``, ``Q = R diag(s)``, ``V = Vt``).  The movie is never
expanded.  For any A, C the best b is ``mbar - A cbar`` (``mbar = mean + Uh Q vbar`` the time mean of X, vbar / cbar the
row means of V / C), so b is not stored while iterating; with ``C~ = C - cbar 1^T`` the objective minus the constant
``||X - mbar 1^T||^2`` is ``J = tr(G H) - 2 sum(C~ o P~)``, ``G = A^T A`` (sparse, host, float64), ``H = C~ C~^T`` (dense,
one pmd_gemm) and ``P~ = A^T Uh Q V~``.

Start: A = the weights with every column scaled to unit 2-norm, C = 0, cbar = 0, then one temporal step.  One outer
iteration:

1. temporal step.  ``B = A^T Uh`` (traces.denoised_factors with the footprints as weights, on U's rows in C pixel order
   so that its bits do not depend on ``pmd.order``) and G are rebuilt on the host, ``Wk = B Q`` is one
   pmd_csr_rows_spmm.  Then ``sweeps`` times, and this is the ordering rule the float64 reference (tests/hals_ref.py)
   follows: the offsets ``o = -Wk vbar + G cbar`` (float64 on the host, from the row means
   cbar as they are now), ``P = Wk V + o 1^T`` in 1024-frame blocks (VtBlocks, pmd_gemm, pmd_roi_combine), one
   ``pmd_hals_sweep`` on C in place, and the new row means cbar (a float64 device reduction).  So the offsets are redone
   once per sweep and lag the traces by one sweep; every sweep lowers J all the same, because the sweep minimises the
   objective for the b of the old cbar and the new cbar only improves on that b.
2. spatial step (``update_footprints``).  C~ is formed in P's buffer, ``N = V C~^T`` and ``H = C~ C~^T`` and
   ``Mt = (Q N)^T`` come from pmd_gemm, and ``sweeps`` calls of ``pmd_hals_pixels`` update, for every pixel of the union
   of supports, the values A[p, k] of the ROIs covering p (the footprints live on the device as pixel-major pairs).
   An ROI whose column became all zero is reported in ``empty`` and frozen: its trace is no longer updated.
3. J in float64 on the host from G, H, B and Mt (``sum(C~ o P~) = sum(B o Mt)``, nothing of length T).

pmd_hals_sweep takes G's rows with their diagonal entry: ``C_k += (P_k - sum_j G_kj C_j) / G_kk`` is the exact
coordinate minimiser only when the sum runs over the whole row.  At the end every non-negative trace is shifted so that
its minimum is 0, and the shift goes into b.

C and P stay on the device for the whole call: ``8 K T`` bytes, the only term that grows with the movie's length
(demix_device_bytes).  Nothing else is of length T except one 1024-frame block of Vt.
"""
import numpy as np
import scipy.sparse

from ._movie import _device_free_bytes
from ._stream import (BLOCK, VtBlocks, _check_count, check_fit, check_pmd, device_context, factor_bytes, scaled_r,
                      upload_f32)
from .traces import denoised_factors, roi_weights

MAX_COVER = 64        # PMD_HALS_MAX_COVER: ROIs covering one pixel (one lane each)


class Demixed:
    """Result of demix: ``traces`` ((K, T) float32), ``footprints`` (scipy.sparse.csr_matrix (K, d1 d2) float32, columns
    numbering pixels in C order), ``background`` ((d1, d2) float32), ``labels`` ((K,)), ``objective`` (float64, J after
    every outer iteration) and ``empty`` ((K,) bool: ROIs whose footprint became all zero)."""

    def __init__(self, traces, footprints, background, labels, objective, empty):
        self.traces, self.footprints, self.background = traces, footprints, background
        self.labels, self.objective, self.empty = labels, objective, empty

    def __repr__(self):
        return "Demixed({} ROIs, {} frames, {} outer iterations{})".format(
            len(self.labels), self.traces.shape[1], len(self.objective),
            ", {} empty".format(int(self.empty.sum())) if self.empty.any() else "")


# ---- host side: tables, offsets, the plan (no device work) ----------------------------------------------------------
def cover_tables(W, max_cover=MAX_COVER):
    """The pixel-major view of the K x D CSR weight matrix ``W`` (roi_weights) for pmd_hals_pixels:

    px       int64 (n_px,)      C-order ids of the pixels some ROI covers (the union of supports), ascending
    cov_ptr  int64 (n_px + 1,)  pairs of pixel q: cov_ptr[q] .. cov_ptr[q + 1]
    cov_k    int32 (n_pairs,)   the ROI of each pair, ascending within a pixel
    perm     int64 (n_pairs,)   the position of each pair's value in W.data

    ValueError when more than ``max_cover`` ROIs cover one pixel."""
    K, D = W.shape
    tag = scipy.sparse.csr_matrix((np.arange(1, W.nnz + 1, dtype=np.float64), W.indices, W.indptr), shape=W.shape).tocsc()
    tag.sort_indices()
    counts = np.diff(tag.indptr)
    if counts.size and int(counts.max()) > max_cover:
        p = int(np.argmax(counts))
        raise ValueError("pixel {} is covered by {} ROIs, at most {} may overlap on one pixel".format(
            p, int(counts[p]), max_cover))
    px = np.nonzero(counts)[0].astype(np.int64)
    return {"px": px, "cov_ptr": np.concatenate([[0], np.cumsum(counts[px])]).astype(np.int64),
            "cov_k": tag.indices.astype(np.int32), "perm": (tag.data - 1).astype(np.int64)}


class _COrderFactors:
    """What traces.denoised_factors reads of a PMDArray, with the rows of U in C pixel order: its sums over the pixels of
    an ROI then run in the same order whatever ``pmd.order`` is, so ``B = A^T Uh`` has the same float64 bits for both."""

    def __init__(self, pmd):
        d1, d2 = (int(x) for x in pmd.shape[1:])
        u_of_c = np.asarray(pmd.row_indices).reshape(-1)
        self.u = pmd.u if pmd.order == "C" else pmd.u[u_of_c]
        self.row_indices = np.arange(d1 * d2).reshape(d1, d2)
        self.var_img, self.mean_img = pmd.var_img, pmd.mean_img


def unit_columns(W):
    """W.data scaled so that every ROI (row of the K x D matrix) has unit 2-norm, float64."""
    norm = np.sqrt(np.asarray(W.multiply(W).sum(axis=1)).reshape(-1))
    return W.data / np.repeat(norm, np.diff(W.indptr))


def time_mean_factors(pmd):
    """(qv, mbar): ``Q vbar`` ((n_cols,) float64) and the time mean ``mbar = mean + Uh Q vbar`` of the denoised movie in
    C pixel order ((D,) float64)."""
    vbar = np.asarray(pmd.v, dtype=np.float64).mean(axis=1) if pmd.v.shape[1] else np.zeros(pmd.v.shape[0])
    qv = (np.asarray(pmd.r, dtype=np.float64) * np.asarray(pmd.s, dtype=np.float64)[None, :]) @ vbar
    u_of_c = np.asarray(pmd.row_indices).reshape(-1)
    std = np.asarray(pmd.var_img, dtype=np.float64).reshape(-1)
    mbar = np.asarray(pmd.mean_img, dtype=np.float64).reshape(-1) + std * np.asarray(pmd.u @ qv).reshape(-1)[u_of_c]
    return qv, mbar


def sweep_offsets(B, G, qv, cbar):
    """o = -Wk vbar + G cbar in float64: ``-B (Q vbar) + G cbar``."""
    return -np.asarray(B @ qv).reshape(-1) + np.asarray(G @ cbar).reshape(-1)


def gram(A, frozen):
    """(G, invd): ``G = A A^T`` of the K x D footprints (CSR float64; explicit zeros dropped, indices ascending, the
    diagonal among them) and 1 / G_kk, 0 for an empty or frozen ROI."""
    G = scipy.sparse.csr_matrix(A @ A.T)
    G.eliminate_zeros()
    G.sort_indices()
    d = G.diagonal()
    return G, np.where((d > 0) & ~frozen, 1.0 / np.where(d > 0, d, 1.0), 0.0)


def demix_device_bytes(*, K, T, n_pairs, n_px, nnz_g, nnz_b, nnz_u, n_rows, n_cols, rank, factors_on_device):
    """Device bytes demix holds for K ROIs on T frames.  The traces C and the products P stay on the device for the whole
    call: 8 K T bytes, the one term that grows with the movie's length.  On top of it one 1024-frame block of Wk Vt and of
    Vt, Wk, N, Mt, H, the CSR matrices G and B, the pixel-major pairs and their tables, and U and R s unless the PMDArray
    already holds them on the device."""
    need = 8 * K * T
    need += 4 * (K * BLOCK + 2 * K * rank + K * n_cols + K * K) + 12 * (nnz_g + nnz_b) + 16 * (K + 1) + 16 * K
    need += 8 * n_pairs + 16 * (n_px + 1)
    need += factor_bytes(n_cols, rank, factors_on_device)
    if not factors_on_device:
        need += 8 * nnz_u + 8 * (n_rows + 1)
    return need + (1 << 20)     # the allocator's rounding of the small arrays


# ---- public entry point --------------------------------------------------------------------------------------------
def demix(pmd, rois, *, outer_iters=3, sweeps=5, update_footprints=True, nonneg_traces=True, device=None, ctx=None):
    """Demix the ROIs ``rois`` (the three forms of traces.roi_weights: (K, d1, d2) weights or booleans, a label image, a
    sparse (K, d1 d2) matrix; weights >= 0, their non-zeros are the supports) on the denoised movie of ``pmd``: a Demixed
    with non-negative ``footprints`` on the given supports, ``traces`` and the static ``background``, such that
    ``footprints^T traces + background`` fits ``mean_img + var_img * (U R diag(s) Vt)`` in the least-squares sense (see
    the module docstring for the iteration).  ``outer_iters`` outer iterations of ``sweeps`` Gauss-Seidel sweeps over
    frames and, with ``update_footprints``, as many over pixels; ``update_footprints=False`` keeps the normalised input
    footprints and only solves for the traces; ``nonneg_traces=False`` lifts the bound on the traces.  No movie is read.

    After ``pmd.to_device()`` its context and uploaded factors are reused; every output bit is the same either way.
    Device memory grows with the movie's length as 8 K T bytes (demix_device_bytes); a plan that does not fit raises
    ValueError.  Argument errors are raised before any device work."""
    check_pmd(pmd)
    outer_iters = _check_count(outer_iters, "outer_iters")
    sweeps = _check_count(sweeps, "sweeps")
    T, d1, d2 = (int(x) for x in pmd.shape)
    W, labels = roi_weights(rois, (d1, d2), pmd.order, "sum")
    if np.any(W.data < 0):
        raise ValueError("rois hold negative weights: footprints are non-negative")
    tabs = cover_tables(W)
    if T == 0:
        raise ValueError("the decomposition has no frames: there is nothing to demix")
    n_cols, rank = (int(x) for x in pmd.r.shape)
    if rank == 0 or n_cols == 0:
        raise ValueError("the decomposition has rank 0: its denoised movie is the mean image, there is nothing to demix")
    if pmd.u.shape[1] != n_cols:
        raise ValueError("U has {} columns, R has {} rows".format(pmd.u.shape[1], n_cols))
    a0 = unit_columns(W).astype(np.float32)
    if not np.all(np.isfinite(a0)):
        raise ValueError("rois hold weights outside the float32 range")
    K = W.shape[0]
    A0 = scipy.sparse.csr_matrix((a0.astype(np.float64), W.indices, W.indptr), shape=W.shape)
    spatial = _COrderFactors(pmd)
    first = (denoised_factors(spatial, A0)[0],) + gram(A0, np.zeros(K, dtype=bool))

    with device_context(pmd, device, ctx) as (ctx, dv):
        need = demix_device_bytes(K=K, T=T, n_pairs=W.nnz, n_px=len(tabs["px"]), nnz_g=first[1].nnz, nnz_b=first[0].nnz,
                                  nnz_u=pmd.u.nnz, n_rows=pmd.u.shape[0], n_cols=n_cols, rank=rank,
                                  factors_on_device=dv is not None)
        check_fit("demix", need, _device_free_bytes(ctx.device))
        C, a, objective, empty, mbar = _solve(ctx, pmd, dv, spatial, first, W, a0, tabs, outer_iters, sweeps,
                                              update_footprints, nonneg_traces)
    # the end of the call: non-negative traces start at 0, the shift goes into the background
    if nonneg_traces:
        C -= C.min(axis=1, keepdims=True)
    A = scipy.sparse.csr_matrix((a, W.indices, W.indptr), shape=W.shape)
    b = mbar - np.asarray(A.T @ C.mean(axis=1, dtype=np.float64)).reshape(-1)
    return Demixed(C, A, b.reshape(d1, d2).astype(np.float32), labels, np.asarray(objective, dtype=np.float64), empty)


def _solve(ctx, pmd, dv, spatial, first, W, a0, tabs, outer_iters, sweeps, update_footprints, nonneg_traces):
    """The iteration on the device; ``first``: (B, G, invd) of the starting footprints.  Returns (C (K, T) float32, the
    footprint values in W.data's order (float32), the objective per outer iteration, the empty flags, mbar)."""
    import torch
    from ._lib import ptr

    dev = ctx.device
    T = int(pmd.shape[0])
    K = W.shape[0]
    n_cols, rank = (int(x) for x in pmd.r.shape)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
    F = 4
    blocks = [(c0, min(T, c0 + BLOCK) - c0) for c0 in range(0, T, BLOCK)]

    qv, mbar = time_mean_factors(pmd)
    rs = scaled_r(ctx, pmd, dv)
    vt = VtBlocks(ctx, pmd, dv)
    C = torch.zeros((K, T), dtype=torch.float32, device=dev)
    P, ct, wk = f32(K, T), f32(K, BLOCK), f32(K, rank)
    N, Mt, H = f32(rank, K), f32(K, n_cols), f32(K, K)
    lo = upload_f32(ctx, np.full(K, 0.0 if nonneg_traces else -np.inf))
    perm = tabs["perm"]
    a = a0.copy()                                  # footprint values in W.data's order
    frozen = np.zeros(K, dtype=bool)
    cbar = np.zeros(K)
    n_px = len(tabs["px"])
    if update_footprints:
        u_of_c = np.asarray(pmd.row_indices).reshape(-1)
        px_row = up(u_of_c[tabs["px"]].astype(np.int32))
        cov_ptr, cov_k = up(tabs["cov_ptr"]), up(tabs["cov_k"])
        scale = upload_f32(ctx, np.asarray(pmd.var_img).reshape(-1)[tabs["px"]])
        if dv is not None:
            u_ptr, u_idx, u_val = dv["indptr"], dv["indices"], dv["data"]
        else:
            u = pmd.u
            u_ptr, u_idx = up(u.indptr.astype(np.int64)), up(u.indices.astype(np.int32) if u.nnz else np.zeros(1, np.int32))
            u_val = upload_f32(ctx, u.data if u.nnz else np.zeros(1))

    def at(t, c0):
        import ctypes

        return ctypes.c_void_p(t.data_ptr() + F * int(c0))

    def factors(known=None):
        """B, G, invd of the footprints as they are (``known``: already formed), and Wk = B Q on the device."""
        if known is None:
            A = scipy.sparse.csr_matrix((a.astype(np.float64), W.indices, W.indptr), shape=W.shape)
            known = (denoised_factors(spatial, A)[0],) + gram(A, frozen)
        B, G, invd = known
        b_ptr = up(B.indptr.astype(np.int64))
        b_idx = up(B.indices.astype(np.int32) if B.nnz else np.zeros(1, np.int32))
        b_val = upload_f32(ctx, B.data if B.nnz else np.zeros(1))
        ctx.call("pmd_csr_rows_spmm", ptr(b_ptr), ptr(b_idx), ptr(b_val), None, K, ptr(rs), rank, rank, ptr(wk), rank)
        return B, G, invd

    def temporal(B, G, invd, cbar):
        g_ptr = up(G.indptr.astype(np.int64))
        g_idx = up(G.indices.astype(np.int32) if G.nnz else np.zeros(1, np.int32))
        g_val = upload_f32(ctx, G.data if G.nnz else np.zeros(1))
        invd_dev = upload_f32(ctx, invd)
        for _ in range(sweeps):
            off = upload_f32(ctx, sweep_offsets(B, G, qv, cbar))
            for c0, m in blocks:
                vt.load(c0, m)
                ctx.call("pmd_gemm", 0, 0, K, m, rank, 1.0, ptr(wk), rank, ptr(vt.buf), BLOCK, 0.0, ptr(ct), BLOCK)
                ctx.call("pmd_roi_combine", K, m, ptr(ct), BLOCK, ptr(off), None, 0, at(P, c0), T, None, 0)
            ctx.call("pmd_hals_sweep", ptr(C), T, ptr(P), T, K, T, ptr(g_ptr), ptr(g_idx), ptr(g_val), ptr(invd_dev),
                     ptr(lo))
            cbar = (torch.sum(C, dim=1, dtype=torch.float64) / T).cpu().numpy()
        return cbar

    def moments(cbar):
        """C~ in P's buffer; N = V C~^T, H = C~ C~^T, Mt = (Q N)^T."""
        neg = upload_f32(ctx, -cbar)
        for i, (c0, m) in enumerate(blocks):
            ctx.call("pmd_roi_combine", K, m, at(C, c0), T, ptr(neg), None, 0, at(P, c0), T, None, 0)
            vt.load(c0, m)
            ctx.call("pmd_gemm", 0, 1, rank, K, m, 1.0, ptr(vt.buf), BLOCK, at(P, c0), T, 0.0 if i == 0 else 1.0, ptr(N), K)
        ctx.call("pmd_gemm", 0, 1, K, K, T, 1.0, ptr(P), T, ptr(P), T, 0.0, ptr(H), K)
        ctx.call("pmd_gemm", 1, 1, K, n_cols, rank, 1.0, ptr(N), K, ptr(rs), rank, 0.0, ptr(Mt), n_cols)

    def footprint_sweeps():
        a_dev = upload_f32(ctx, a[perm])
        frozen_dev = up(frozen.astype(np.int32))
        for _ in range(sweeps):
            ctx.call("pmd_hals_pixels", n_px, ptr(px_row), ptr(cov_ptr), ptr(cov_k), ptr(a_dev), ptr(u_ptr), ptr(u_idx),
                     ptr(u_val), ptr(scale), ptr(Mt), n_cols, ptr(H), K, ptr(frozen_dev))
        ctx.sync()
        a[perm] = a_dev.cpu().numpy()

    B, G, invd = factors(first)
    cbar = temporal(B, G, invd, cbar)
    objective = []
    for _ in range(outer_iters):
        cbar = temporal(B, G, invd, cbar)
        moments(cbar)
        if update_footprints:
            footprint_sweeps()
            nz = np.add.reduceat((a != 0).astype(np.int64), W.indptr[:-1]) > 0
            frozen |= ~nz
            B, G, invd = factors()
        ctx.sync()
        H64, Mt64 = H.cpu().numpy().astype(np.float64), Mt.cpu().numpy().astype(np.float64)
        objective.append(float(G.multiply(H64).sum() - 2.0 * B.multiply(Mt64).sum()))
    ctx.sync()
    return C.cpu().numpy(), a, objective, frozen, mbar
