"""Plain NumPy / SciPy statements of the superpixel initialisation (localmd_amd/superpixels.py, csrc/superpixel.hip), on an
expanded (T, d1, d2) float32 movie: the rectified movie, the six sums as strict sequential fp64 chains, the float64
finish, the edge byte, the connected components through scipy.sparse.csgraph and the whole ``superpixels_ref``.  Written
pixel pair by pixel pair where the package shifts whole images; nothing here is imported from the package."""
import numpy as np
import scipy.sparse
import scipy.sparse.csgraph

FORWARD = ((0, 1), (1, -1), (1, 0), (1, 1))      # bit 0 E, bit 1 SW, bit 2 S, bit 3 SE


def rectified(X, thr):
    """y = v > thr ? fl32(v - thr) : 0 on the (T, d1, d2) movie X taken as float32; NaN compares false."""
    X = np.asarray(X).astype(np.float32)
    thr = np.asarray(thr, dtype=np.float32)[None]
    with np.errstate(invalid="ignore"):
        return np.where(X > thr, (X - thr).astype(np.float32), np.float32(0)).astype(np.float32)


def chain(terms):
    """The strict sequential fp64 sum over axis 0, started from the first term (0 + x = x exactly)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.cumsum(np.asarray(terms, dtype=np.float64), axis=0)[-1]


def neighbour(y, di, dj):
    """z[..., i, j] = y[..., i + di, j + dj], 0 outside the image."""
    d1, d2 = y.shape[-2:]
    z = np.zeros_like(y)
    for i in range(d1):
        for j in range(d2):
            if 0 <= i + di < d1 and 0 <= j + dj < d2:
                z[..., i, j] = y[..., i + di, j + dj]
    return z


def moments(y, start=None):
    """(6, d1 d2) float64: S1, S2, E, SW, S, SE of the rectified (T, d1, d2) movie y, each a chain in frame order that
    goes on from ``start``."""
    y64 = np.asarray(y, dtype=np.float32).astype(np.float64)
    T, d1, d2 = y64.shape
    with np.errstate(invalid="ignore", over="ignore"):
        terms = [y64, y64 * y64] + [y64 * neighbour(y64, di, dj) for di, dj in FORWARD]
    out = np.empty((6, d1 * d2))
    for k, t in enumerate(terms):
        t = t.reshape(T, -1)
        if start is not None:
            t = np.concatenate([np.asarray(start, np.float64)[k][None], t])
        out[k] = chain(t)
    return out


def moments_at(y, lengths):
    """{n: moments(y[:n])} for the lengths asked for, from one pass: the n-th partial sum of a chain is the chain of the
    first n terms."""
    y64 = np.asarray(y, dtype=np.float32).astype(np.float64)
    T, d1, d2 = y64.shape
    out = {n: np.empty((6, d1 * d2)) for n in lengths}
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(6):
            t = y64 if k == 0 else y64 * (y64 if k == 1 else neighbour(y64, *FORWARD[k - 2]))
            c = np.cumsum(t.reshape(T, -1), axis=0)
            for n in lengths:
                out[n][k] = c[n - 1]
    return out


def finish(mom, T, d1, d2):
    """(4, d1, d2) float64 rho, pair by pair: (T Sq - S1_p S1_q) / sqrt(var_p var_q), var = T S2 - S1^2; 0 when a
    variance is at or below 3 (T + 2) 2^-53 T S2 or the neighbour lies outside."""
    m = np.asarray(mom, np.float64).reshape(6, d1, d2)
    T = float(T)
    floor = 3.0 * (T + 2.0) * 2.0 ** -53
    rho = np.zeros((4, d1, d2))
    with np.errstate(all="ignore"):
        var = T * m[1] - m[0] * m[0]
        dead = var <= floor * T * m[1]
        for b, (di, dj) in enumerate(FORWARD):
            for i in range(d1):
                for j in range(d2):
                    qi, qj = i + di, j + dj
                    if not (0 <= qi < d1 and 0 <= qj < d2) or dead[i, j] or dead[qi, qj]:
                        continue
                    rho[b, i, j] = (T * m[2 + b, i, j] - m[0, i, j] * m[0, qi, qj]) / np.sqrt(var[i, j] * var[qi, qj])
    return rho


def edge_byte(rho, cut_off):
    """bit b of pixel (i, j): its forward neighbour b lies inside the image and rho is finite and > cut_off."""
    _, d1, d2 = rho.shape
    e = np.zeros((d1, d2), np.uint8)
    for b, (di, dj) in enumerate(FORWARD):
        for i in range(d1):
            for j in range(d2):
                if 0 <= i + di < d1 and 0 <= j + dj < d2 and np.isfinite(rho[b, i, j]) and rho[b, i, j] > cut_off:
                    e[i, j] |= np.uint8(1 << b)
    return e


def components(edges, d1, d2):
    """(d1, d2) int32: the smallest pixel index of every pixel's component; bits that point outside the image are
    ignored."""
    e = np.asarray(edges, np.uint8).reshape(d1, d2)
    ii, jj = np.mgrid[0:d1, 0:d2]
    rows, cols = [], []
    for b, (di, dj) in enumerate(FORWARD):
        on = ((e >> b) & 1).astype(bool) & (ii + di < d1) & (jj + dj >= 0) & (jj + dj < d2)
        rows.append((ii[on] * d2 + jj[on]).ravel())
        cols.append(((ii[on] + di) * d2 + jj[on] + dj).ravel())
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    D = d1 * d2
    g = scipy.sparse.coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(D, D))
    _, comp = scipy.sparse.csgraph.connected_components(g, directed=False)
    least = np.full(comp.max() + 1, D, np.int64)
    np.minimum.at(least, comp, np.arange(D))
    return least[comp].astype(np.int32).reshape(d1, d2)


def number(root, min_size, max_size=None):
    """(labels, sizes, n_components): kept components 1 .. K in ascending order of their root."""
    flat = np.asarray(root).reshape(-1)
    labels, sizes, k = np.zeros(flat.shape, np.int32), [], 0
    roots = sorted(set(flat.tolist()))
    for r in roots:
        members = flat == r
        size = int(members.sum())
        if size >= min_size and (max_size is None or size <= max_size):
            k += 1
            labels[members] = k
            sizes.append(size)
    return labels.reshape(np.asarray(root).shape), np.asarray(sizes, np.int64), len(roots)


def correlation(rho):
    """(d1, d2) float32: max over the 8 neighbours of the finite rho, from 0."""
    _, d1, d2 = rho.shape
    out = np.zeros((d1, d2))
    for b, (di, dj) in enumerate(FORWARD):
        for i in range(d1):
            for j in range(d2):
                r = rho[b, i, j]
                if np.isfinite(r) and 0 <= i + di < d1 and 0 <= j + dj < d2:
                    out[i, j] = max(out[i, j], r)
                    out[i + di, j + dj] = max(out[i + di, j + dj], r)
    return out.astype(np.float32)


def median32(A):
    """The float32 "linear" median over axis 0 of float32 values: with h = (T - 1) / 2 the order statistics lo = floor(h)
    and hi = ceil(h), float32(lo + (hi - lo) (h - floor(h))) formed in float64 and rounded once (quantile_images)."""
    s = np.sort(np.asarray(A, dtype=np.float32), axis=0).astype(np.float64)
    h = 0.5 * (s.shape[0] - 1)
    lo, hi = int(np.floor(h)), int(np.ceil(h))
    return (s[lo] + (s[hi] - s[lo]) * (h - lo)).astype(np.float32)


def threshold(X, th):
    """fl32(fl32(float32(th) * mad) + med): med = median32 over the frames, mad = median32 of |x - med| with the
    difference in fp32."""
    X = np.asarray(X).astype(np.float32)
    med = median32(X)
    mad = median32(np.abs((X - med[None]).astype(np.float32)))
    return (np.float32(th) * mad).astype(np.float32) + med


def superpixels_ref(X, th=2.0, cut_off=0.9, min_size=10, max_size=None, threshold_image=None):
    """dict(labels, sizes, correlation, threshold, n_components, rho, edges) of the (T, d1, d2) float32 movie X."""
    X = np.asarray(X).astype(np.float32)
    T, d1, d2 = X.shape
    thr = threshold(X, th) if threshold_image is None else np.asarray(threshold_image, np.float32)
    rho = finish(moments(rectified(X, thr)), T, d1, d2)
    edges = edge_byte(rho, cut_off)
    labels, sizes, n = number(components(edges, d1, d2), min_size, max_size)
    return {"labels": labels, "sizes": sizes, "correlation": correlation(rho), "threshold": thr, "n_components": n,
            "rho": rho, "edges": edges}
