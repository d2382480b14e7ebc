"""Plain NumPy / SciPy statements of what localmd_amd.grow computes, written pair by pair and pixel by pixel:

* ``y_column``: the fp32 chain of pmd_roi_window_moments_accumulate for one pair, operation by operation;
* ``pair_moments``: its three fp64 chains (superpixel_ref.chain), optionally continued from a stored state;
* ``finish``: correlation and slope with the variance floor;
* ``windows`` / ``tables``: bounding boxes and the pair and others tables by brute force;
* ``grow_rule``: the growing rule on one window; ``merge``: merge_rois; ``grow_ref``: grow_rois on an expanded movie.
"""
import numpy as np
import scipy.ndimage

from tests.superpixel_ref import chain

U53 = 2.0 ** -53


def y_column(x, others, Ct):
    """(n,) float32: x (n,) of any element type taken as float32, minus fl32(a * Ct[:, l]) for (l, a) of ``others`` in
    order, every operation rounded to fp32 on its own.  Ct: (n, K) float32."""
    y = np.asarray(x).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for l, a in others:
            prod = (np.float32(a) * Ct[:, l].astype(np.float32)).astype(np.float32)
            y = (y - prod).astype(np.float32)
    return y


def pair_moments(X, Ct, pair_px, pair_k, others, start=None):
    """(3, n_pairs) float64: Sy, Syy, Syc of every pair over the frames of X ((n, D)), each a chain in frame order that
    goes on from ``start``.  others[i]: the (l, a) of pair i in stored order."""
    n_pairs = len(pair_px)
    out = np.empty((3, n_pairs))
    for i in range(n_pairs):
        y = y_column(X[:, pair_px[i]], others[i], Ct).astype(np.float64)
        c = Ct[:, pair_k[i]].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            for s, terms in enumerate((y, y * y, y * c)):
                out[s, i] = chain(terms if start is None else np.concatenate([[start[s][i]], terms]))
    return out


def finish(mom, T, Sc, Scc):
    """(rho, beta) per pair, one at a time."""
    n = np.asarray(mom).shape[1]
    rho, beta = np.zeros(n), np.zeros(n)
    T = float(T)
    floor = 3.0 * (T + 2.0) * U53
    with np.errstate(all="ignore"):
        for i in range(n):
            Sy, Syy, Syc = (np.float64(mom[s][i]) for s in range(3))
            var_y = T * Syy - Sy * Sy
            var_c = T * np.float64(Scc[i]) - np.float64(Sc[i]) * np.float64(Sc[i])
            cov = T * Syc - Sy * np.float64(Sc[i])
            beta[i] = cov / var_c
            if var_y > floor * T * Syy and var_c > floor * T * np.float64(Scc[i]):
                rho[i] = cov / np.sqrt(var_y * var_c)
    return rho, beta


def windows(A, d1, d2, halo):
    """{k: (i0, i1, j0, j1)} of the ROIs of the dense (K, D) ``A`` with a support."""
    out = {}
    for k in range(A.shape[0]):
        ii = [p // d2 for p in range(d1 * d2) if A[k, p] > 0]
        jj = [p % d2 for p in range(d1 * d2) if A[k, p] > 0]
        if ii:
            out[k] = (max(0, min(ii) - halo), min(d1, max(ii) + halo + 1), max(0, min(jj) - halo), min(d2, max(jj) + halo + 1))
    return out


def tables(A, win, movable, d2):
    """(pair_px, pair_k, others) by a double loop: the pairs of the movable ROIs in (ROI, pixel) order; others[i] the
    (l, A[l, p]) with l != k and A[l, p] != 0 in ascending l."""
    pair_px, pair_k, others = [], [], []
    for k in range(A.shape[0]):
        if not movable[k]:
            continue
        i0, i1, j0, j1 = win[k]
        for i in range(i0, i1):
            for j in range(j0, j1):
                p = i * d2 + j
                pair_px.append(p)
                pair_k.append(k)
                others.append([(l, A[l, p]) for l in range(A.shape[0]) if l != k and A[l, p] != 0])
    return pair_px, pair_k, others


def grow_rule(rho, seed, corr_th, shrink=True, max_size=None):
    """(support or None, th, status) on one window."""
    th = float(corr_th)
    while True:
        cand = np.zeros(rho.shape, bool)
        for idx in np.ndindex(*rho.shape):
            cand[idx] = bool(np.isfinite(rho[idx]) and rho[idx] > th)
        lab, n = scipy.ndimage.label(cand, structure=np.ones((3, 3)))
        new = np.zeros(rho.shape, bool)
        for c in range(1, n + 1):
            if (seed & (lab == c)).any():
                new |= lab == c
        if not new.any():
            return None, th, "lost"
        if not shrink:
            new |= seed
        if max_size is None or new.sum() <= max_size:
            return new, th, "grown"
        if th + 0.1 < 1:
            th = th + 0.1
        else:
            return None, th, "oversize"


def grow_ref(X, A, C, d1, d2, *, corr_th=0.6, halo=6, shrink=True, max_size=None, fixed=None, max_window=16384):
    """grow_rois on the expanded movie X ((T, d1, d2), any element type), the dense (K, D) float32 footprints A and the
    (K, T) float32 traces C.  Returns a dict: ``rows`` ({k: (indices, float32 values)} of the ROIs with a support),
    ``status``, ``threshold``, ``added``, ``removed`` per ROI, ``rho`` / ``beta`` ({k: (h, w) float64} of the ROIs that
    had pairs), ``win`` and ``margin``, the smallest |rho - corr_th| over the pairs with rho != 0."""
    A = np.asarray(A, dtype=np.float32)
    C = np.asarray(C, dtype=np.float32)
    K, D = A.shape
    T = X.shape[0]
    X2 = np.asarray(X).reshape(T, D)
    Ct = np.ascontiguousarray(C.T)
    fixed = np.zeros(K, bool) if fixed is None else np.asarray(fixed, bool)
    win = windows(A, d1, d2, halo)
    status = []
    for k in range(K):
        if k not in win:
            status.append("empty")
        elif fixed[k] or (win[k][1] - win[k][0]) * (win[k][3] - win[k][2]) > max_window:
            status.append("fixed")
        else:
            status.append("grown")
    movable = [s == "grown" for s in status]
    pair_px, pair_k, others = tables(A, win, movable, d2)
    mom = pair_moments(X2, Ct, pair_px, pair_k, others)
    Sc = [np.sum(np.ascontiguousarray(C[k], dtype=np.float64)) for k in range(K)]
    Scc = [np.sum(np.ascontiguousarray(C[k], dtype=np.float64) ** 2) for k in range(K)]
    rho, beta = finish(mom, T, [Sc[k] for k in pair_k], [Scc[k] for k in pair_k])
    out = {"rows": {}, "status": status, "threshold": np.full(K, float(corr_th)), "added": np.zeros(K, np.int64),
           "removed": np.zeros(K, np.int64), "rho": {}, "beta": {}, "win": win,
           "margin": float(np.abs(rho[rho != 0] - corr_th).min()) if (rho != 0).any() else np.inf}
    at = 0
    for k in range(K):
        if k not in win:
            continue
        sup = np.nonzero(A[k] > 0)[0]
        out["rows"][k] = (sup.astype(np.int64), A[k, sup].astype(np.float32))
        if not movable[k]:
            continue
        i0, i1, j0, j1 = win[k]
        h, w = i1 - i0, j1 - j0
        r, b = rho[at:at + h * w].reshape(h, w), beta[at:at + h * w].reshape(h, w)
        at += h * w
        out["rho"][k], out["beta"][k] = r, b
        seed = (A[k].reshape(d1, d2) > 0)[i0:i1, j0:j1]
        new, out["threshold"][k], status[k] = grow_rule(r, seed, corr_th, shrink, max_size)
        if new is None:
            continue
        idx, val = [], []
        for i in range(h):
            for j in range(w):
                if new[i, j]:
                    p = (i0 + i) * d2 + j0 + j
                    idx.append(p)
                    val.append(A[k, p] if seed[i, j] and not b[i, j] > 0 else np.float32(b[i, j]))
        out["rows"][k] = (np.array(idx, np.int64), np.array(val, np.float32))
        out["added"][k], out["removed"][k] = int((new & ~seed).sum()), int((seed & ~new).sum())
    return out


def merge(A, C, corr_th=0.8, overlap_th=0.6, fixed=None):
    """(rows, groups) of merge_rois on the dense (K, D) float32 A and the (K, T) traces C: a union-find over all pairs."""
    A = np.asarray(A, dtype=np.float32)
    C64 = np.asarray(C, dtype=np.float64)
    K = A.shape[0]
    fixed = np.zeros(K, bool) if fixed is None else np.asarray(fixed, bool)
    parent = list(range(K))

    def root(x):
        while parent[x] != x:
            x = parent[x]
        return x

    S = A > 0
    for k in range(K):
        for l in range(k + 1, K):
            both = int((S[k] & S[l]).sum())
            if not both or fixed[k] or fixed[l] or not both / min(S[k].sum(), S[l].sum()) > overlap_th:
                continue
            with np.errstate(all="ignore"):
                r = np.corrcoef(C64[k], C64[l])[0, 1]
            if r > corr_th:
                a, b = sorted((root(k), root(l)))
                parent[b] = a
    groups = [[l for l in range(K) if root(l) == k] for k in range(K) if root(k) == k]
    rows = []
    for g in groups:
        if len(g) == 1:
            rows.append(A[g[0]])
        else:
            acc = np.zeros(A.shape[1])
            for k in g:
                acc += A[k].astype(np.float64) * np.sqrt(((C64[k] - C64[k].mean()) ** 2).sum())
            rows.append(acc.astype(np.float32))
    return np.stack(rows), groups
