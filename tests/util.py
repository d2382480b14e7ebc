"""Shared helpers for the parity tests (test infrastructure only)."""
import os

import numpy as np


def context_under(env, device_index=0):
    """A Context of its own, created with the variables of ``env`` set (a value of None: unset).  The library reads its
    PMD_* route switches when a context is created and keeps them for that context, so a test that wants a route gets it
    from a context made for it; the environment is put back before this returns.  The caller closes the context."""
    from localmd_amd._lib import Context

    saved = {name: os.environ.get(name) for name in env}
    try:
        for name, value in env.items():
            if value is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = value
        return Context(device_index)
    finally:
        for name, value in saved.items():
            if value is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = value


class DeviceSource:
    """Random source for the oracle that returns the matrices the HIP library generates
    (pmd_rng_normal), so both sides consume bit-identical Gaussian inputs."""

    def __init__(self, ctx, seed):
        self.ctx = ctx
        self.seed = int(seed)

    def _fill(self, stream, index, rows, cols):
        import torch
        from localmd_amd._lib import ptr

        out = torch.empty((rows, cols), dtype=torch.float32, device=self.ctx.device)
        self.ctx.call("pmd_rng_normal", self.seed, stream, index, 0, 1, rows, cols, 0, ptr(out), cols, 0)
        self.ctx.sync()
        return out.cpu().numpy()

    def omega(self, stream, index, rows, cols):
        return self._fill(stream, index, rows, cols)

    def noise(self, index, d1, d2, t):
        z = self._fill(2, index, d1 * d2, t)
        return z.reshape(d2, d1, t).transpose(1, 0, 2)


def reference_sparse_u(ut, ranks, origins, fov_shape, block, order, block_weights):
    """The reference's sparse assembly (decomposition.py:812-853), literally: per tile the float64 components times the
    pyramid weights as COO triplets, the accumulated weights, then the row normalisation as a diagonal product (which drops
    exact zeros).  ut: (n_tiles, component rows, >= b1 * b2) float32, tile pixel q = il + b1 * jl.  Returns the CSR matrix
    (D x sum(ranks), sorted indices) with rows in `order` of the field of view."""
    from scipy.sparse import coo_matrix, diags

    d1, d2 = fov_shape
    b1, b2 = block
    d = b1 * b2
    fov = np.arange(d1 * d2).reshape((d1, d2), order=order)
    rows_l, cols_l, vals_l, col, cw = [], [], [], 0, np.zeros((d1, d2))
    for t, (k, j) in enumerate(origins):
        rk = int(ranks[t])
        sp = ut[t, :rk, :d].T.reshape((b1, b2, rk), order="F").astype(np.float64) * block_weights[:, :, None]
        cw[k:k + b1, j:j + b2] += block_weights
        ridx = fov[k:k + b1, j:j + b2][:, :, None] + np.zeros((1, 1, rk))
        cidx = np.zeros_like(ridx) + np.arange(col, col + rk)[None, None, :]
        rows_l += ridx.flatten().tolist()
        cols_l += cidx.flatten().tolist()
        vals_l += sp.flatten().tolist()
        col += rk
    ref = coo_matrix((vals_l, (rows_l, cols_l)), shape=(d1 * d2, col))
    wnd = np.zeros(d1 * d2)
    wnd[fov.flatten(order=order)] = cw.flatten(order=order)
    ref = diags([(1 / wnd).ravel()], [0]).dot(ref).tocsr()
    ref.sort_indices()
    return ref


def sign_align(a, b, axis=0):
    """Flip the sign of each column (axis=0) / row (axis=1) of ``a`` to best match ``b``."""
    dots = np.sum(a * b, axis=axis, keepdims=True)
    return a * np.where(dots < 0, -1.0, 1.0)


def rel_err(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) /
                 max(np.linalg.norm(np.asarray(b, dtype=np.float64)), 1e-300))


def degenerate_pmds(pmd):
    """{"no_columns", "rank_zero"}: PMDArrays with the shape, order and statistics of ``pmd`` whose denoised movie is the
    mean image in every frame: a U without columns, and the U of ``pmd`` with factors of rank 0."""
    import scipy.sparse
    from localmd_amd.pmdarray import PMDArray

    T, d1, d2 = pmd.shape
    n_cols, f32 = pmd.u.shape[1], np.float32

    def make(u, k):
        return PMDArray(u, np.zeros((k, 0), f32), np.zeros(0, f32), np.zeros((0, T), f32), (T, d1, d2), pmd.order,
                        pmd.mean_img, pmd.var_img)

    return {"no_columns": make(scipy.sparse.csr_matrix((d1 * d2, 0), dtype=f32), 0), "rank_zero": make(pmd.u, n_cols)}
