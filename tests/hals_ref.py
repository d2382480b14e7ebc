"""NumPy statements of the demixing solver (localmd_amd/demix.py, csrc/hals.hip); holds no test itself.

* ``hals_sweep``: pmd_hals_sweep operation by operation in the dtype of its arrays.  On float32 arrays every product, every
  subtraction and the final step are rounded on their own in the kernel's order, so the result equals the kernel's bit
  for bit; on float64 arrays it is the reference.
* ``hals_pixels``: the update order of pmd_hals_pixels (pairs of a pixel in ascending order, each reading the newest
  values) in the dtype of ``a``.  The kernel sums over lanes and a butterfly, NumPy in its own order: float64 is the
  reference, float32 an estimate of the fp32 error, not the kernel's bits.
* ``demix_ref``: the whole iteration of demix() on an expanded movie X (D x T), dense, with the ordering rules of the
  module: one temporal step from C = 0 first; then per outer iteration a temporal step (per sweep: offsets from the
  current row means, one sweep, new row means), a spatial step, the objective; the shift of non-negative traces at the
  end.  What demix() keeps in float64 on the host (G, the offsets, the row means, the objective) is float64 here too;
  ``dtype=np.float32`` rounds what the device holds in fp32.
"""
import numpy as np


def hals_sweep(C, P, indptr, indices, data, invd, lo):
    """One sweep on C ((K, ldc) rows, updated in place over all its columns) with P (same shape), the CSR rows of G (the
    diagonal stored), invd and lo; all of C's dtype."""
    dt = C.dtype
    assert P.dtype == dt and data.dtype == dt and invd.dtype == dt and lo.dtype == dt
    for k in range(len(invd)):
        if invd[k] == 0:
            continue
        acc = P[k].copy()
        for i in range(int(indptr[k]), int(indptr[k + 1])):
            prod = data[i] * C[indices[i]]
            acc = acc - prod
        step = acc * invd[k]
        v = C[k] + step
        C[k] = np.where(v < lo[k], lo[k], v)
    return C


def gauss_seidel_pairs(av, sy, Hs, skip):
    """The pairs of one pixel: av[j] = max(0, av[j] + (sy[j] - av . Hs[:, j]) / Hs[j, j]) for ascending j, in place."""
    zero = av.dtype.type(0)
    for j in range(len(av)):
        if skip[j] or Hs[j, j] == 0:
            continue
        dot = av @ Hs[:, j]
        v = av[j] + (sy[j] - dot) / Hs[j, j]
        av[j] = zero if v < 0 else v
    return av


def hals_pixels(a, px_row, cov_ptr, cov_k, U, scale, Mt, H, frozen):
    """pmd_hals_pixels on the pair values ``a`` (in place, its dtype): U a scipy CSR matrix, Mt (K, n_cols), H (K, K)."""
    dt = a.dtype
    Mt, H, scale = Mt.astype(dt), H.astype(dt), scale.astype(dt)
    for q in range(len(px_row)):
        j0, j1 = int(cov_ptr[q]), int(cov_ptr[q + 1])
        ks = cov_k[j0:j1]
        s, e = U.indptr[px_row[q]], U.indptr[px_row[q] + 1]
        idx, val = U.indices[s:e], U.data[s:e].astype(dt)
        sy = scale[q] * (Mt[ks][:, idx] @ val)
        a[j0:j1] = gauss_seidel_pairs(a[j0:j1].copy(), sy.astype(dt), H[np.ix_(ks, ks)], frozen[ks] != 0)
    return a


def normalise_columns(A0):
    """Columns of the (D, K) weights scaled to unit 2-norm, float64."""
    A = np.asarray(A0, dtype=np.float64)
    return A / np.sqrt((A * A).sum(axis=0, keepdims=True))


def gram_csr(A64, frozen):
    """(indptr, indices, data, invd) of G = A^T A in float64: the nonzeros of each row in ascending order, the diagonal
    among them; invd = 1 / G_kk, 0 for an empty or frozen column."""
    G = A64.T @ A64
    K = G.shape[0]
    indptr, indices, data = [0], [], []
    for k in range(K):
        nz = np.nonzero(G[k])[0]
        indices.extend(nz)
        data.extend(G[k, nz])
        indptr.append(len(indices))
    d = np.diag(G)
    invd = np.where((d > 0) & ~frozen, 1.0 / np.where(d > 0, d, 1.0), 0.0)
    return G, np.asarray(indptr, np.int64), np.asarray(indices, np.int32), np.asarray(data, np.float64), invd


def shift_traces(C, A, mbar, nonneg):
    """The end of a call, float64: every non-negative trace moved so that its minimum is 0, the move going into the
    background b = mbar - A cbar.  Returns (C, b)."""
    C = np.array(C, dtype=np.float64)
    if nonneg and C.shape[1]:
        C -= C.min(axis=1, keepdims=True)
    cbar = C.mean(axis=1) if C.shape[1] else np.zeros(len(C))
    return C, mbar - A @ cbar


def demix_ref(X, A0, supports, outer_iters=3, sweeps=5, update_footprints=True, nonneg_traces=True, dtype=np.float64):
    """X (D, T) float64, A0 (D, K) >= 0 weights, supports (D, K) bool.  Returns a dict: traces (K, T), footprints (D, K),
    background (D,), objective (outer_iters,), empty (K,), all float64 values (computed in ``dtype`` where the device
    holds fp32), and ``residual``: ||X - A C - b 1^T||_F^2 per outer iteration, evaluated directly."""
    dt = np.dtype(dtype).type
    X = np.asarray(X, dtype=np.float64)
    D, T = X.shape
    supports = np.asarray(supports, dtype=bool)
    K = supports.shape[1]
    mbar = X.mean(axis=1)
    Xt = (X - mbar[:, None]).astype(dt)
    A = (normalise_columns(A0) * supports).astype(dt)
    C = np.zeros((K, T), dtype=dt)
    cbar = np.zeros(K)
    frozen = np.zeros(K, dtype=bool)
    lo = np.full(K, 0.0 if nonneg_traces else -np.inf).astype(dt)
    px = np.nonzero(supports.any(axis=1))[0]

    def temporal(cbar):
        A64 = A.astype(np.float64)
        G, indptr, indices, data, invd = gram_csr(A64, frozen)
        Pt = A.T @ Xt                                   # A^T (X - mbar 1^T), the device's Wk V - Wk vbar
        for _ in range(sweeps):
            o = G @ cbar
            hals_sweep(C, Pt + o.astype(dt)[:, None], indptr, indices, data.astype(dt), invd.astype(dt), lo)
            cbar = C.astype(np.float64).mean(axis=1)
        return cbar

    cbar = temporal(cbar)
    objective, residual = [], []
    for _ in range(outer_iters):
        cbar = temporal(cbar)
        Ct = (C + (-cbar).astype(dt)[:, None]).astype(dt)
        H = Ct @ Ct.T
        S = Xt @ Ct.T                                   # (D, K): the Sy of every pixel and ROI
        if update_footprints:
            for _ in range(sweeps):
                for p in px:
                    ks = np.nonzero(supports[p])[0]
                    A[p, ks] = gauss_seidel_pairs(A[p, ks].copy(), S[p, ks], H[np.ix_(ks, ks)], frozen[ks])
            frozen |= ~(A != 0).any(axis=0)
        A64 = A.astype(np.float64)
        G = A64.T @ A64
        objective.append(float((G * H.astype(np.float64)).sum() - 2.0 * (A64 * S.astype(np.float64)).sum()))
        b = mbar - A64 @ cbar
        residual.append(float(((X - A64 @ C.astype(np.float64) - b[:, None]) ** 2).sum()))
    A64 = A.astype(np.float64)
    Cs, b = shift_traces(C, A64, mbar, nonneg_traces)
    return {"traces": Cs, "footprints": A64, "background": b, "objective": np.asarray(objective),
            "residual": np.asarray(residual), "empty": frozen.copy(), "unshifted": C.astype(np.float64)}
