"""
Plain NumPy reference of the diagnostic-image kernels (csrc/diag.hip, csrc/diag_fused.hip) and of the two expansion
primitives (csrc/expand.hip): the same operations written as array expressions, in int64 where every input has an integer
dtype (the sums are then exact) and in float64 otherwise.  No torch, no device.  tests/test_diag_ref.py ties the moment
layout and the image formulas to oracle/diag_oracle.py.

Movies are (T, d1, d2); moments are (rows, D) with D = d1 * d2 and pixel p = i * d2 + j.  ``absolute=True`` replaces every
term of every sum by its absolute value (always float64): the sum of |terms| that a rounding-error bound is stated in.
"""
import numpy as np

# the 8 neighbours in the row-major (di, dj) order of include/pmd_hip.h
OFFSETS = [(di, dj) for di in (-1, 0, 1) for dj in (-1, 0, 1) if (di, dj) != (0, 0)]


def _wide(*arrays):
    """The arrays in int64 if all of them have an integer dtype, else in float64."""
    arrays = [np.asarray(a) for a in arrays]
    kind = np.int64 if all(a.dtype.kind in "iu" for a in arrays) else np.float64
    return [a.astype(kind) for a in arrays]


def neighbour_index(d1, d2):
    """(q (8, D) clamped neighbour pixel, exists (8, D) bool): neighbour k of pixel p = (i, j) is (i + di, j + dj), moved to
    the nearest pixel of the field of view when it is outside (as the moments kernels do)."""
    i, j = np.divmod(np.arange(d1 * d2), d2)
    q = np.empty((8, d1 * d2), dtype=np.int64)
    exists = np.empty((8, d1 * d2), dtype=bool)
    for k, (di, dj) in enumerate(OFFSETS):
        ii, jj = i + di, j + dj
        exists[k] = (ii >= 0) & (ii < d1) & (jj >= 0) & (jj < d2)
        q[k] = np.clip(ii, 0, d1 - 1) * d2 + np.clip(jj, 0, d2 - 1)
    return q, exists


def _moments_of(x, d1, d2, absolute):
    """(10, D): sum x, sum x^2, sum x_p x_q over the frames of the shifted traces x (T, D)."""
    q, _ = neighbour_index(d1, d2)
    if absolute:
        x = np.abs(x.astype(np.float64))
    out = np.empty((10, d1 * d2), dtype=x.dtype)
    out[0] = x.sum(axis=0)
    out[1] = (x * x).sum(axis=0)
    for k in range(8):
        out[2 + k] = (x * x[:, q[k]]).sum(axis=0)
    return out


def neighbour_moments(a, b=None, ref=None, absolute=False):
    """(moments (10, D), exists (8, D)) of x = a - b (b may be None), every trace shifted by ``ref`` (D values; None: frame
    0 of x).  Rows: sum x, sum x^2, then sum x_p x_q for the 8 neighbours q, clamped into the field of view; exists[k] tells
    which of those are real neighbours."""
    T, d1, d2 = np.shape(a)
    if b is None:
        (x,) = _wide(a)
    else:
        x, y = _wide(a, b)
        x = x - y
    x = x.reshape(T, d1 * d2)
    r = x[0] if ref is None else np.asarray(ref).reshape(-1).astype(x.dtype)
    return _moments_of(x - r[None, :], d1, d2, absolute), neighbour_index(d1, d2)[1]


def lag_moments(a, ref, lag, absolute=False):
    """(5, D) in the layout of lag_moments_kernel: with x = a[lag:] - ref and y = a[:-lag] - ref, sum x, sum x^2, sum y,
    sum y^2, sum x y.  ref: D values, None = frame 0."""
    (a,) = _wide(a)
    a = a.reshape(a.shape[0], -1)
    if not 1 <= lag < a.shape[0]:
        raise ValueError("need 1 <= lag < frames")
    r = a[0] if ref is None else np.asarray(ref).reshape(-1).astype(a.dtype)
    x, y = a[lag:] - r[None, :], a[:-lag] - r[None, :]
    if absolute:
        x, y = np.abs(x.astype(np.float64)), np.abs(y.astype(np.float64))
    return np.stack([x.sum(axis=0), (x * x).sum(axis=0), y.sum(axis=0), (y * y).sum(axis=0), (x * y).sum(axis=0)])


def fused_moments(y, w, mean, lag, ref=None, absolute=False):
    """(moments (35, D), frame_ss (T,)) of pmd_diag_fused_accumulate over the whole movie: with r = (y - mean) - w, the
    neighbour moments of y, of w and of r and the lag moments of y, every trace shifted by its value in frame 0 (or by
    ref (3, D) = the shifts of y, w and r); frame_ss[t] = sum over the pixels of r_t^2, not shifted."""
    T, d1, d2 = np.shape(y)
    y, w, mean = _wide(y, w, mean)
    ym = y - mean[None]
    r = ym - w
    sh = [None, None, None] if ref is None else list(np.asarray(ref))
    mom = np.concatenate([neighbour_moments(y, None, sh[0], absolute)[0], neighbour_moments(w, None, sh[1], absolute)[0],
                          neighbour_moments(ym, w, sh[2], absolute)[0], lag_moments(y, sh[0], lag, absolute)])
    return mom, (r * r).reshape(T, -1).sum(axis=1)


def neighbour_image(num, den, T, d1, d2, kind, mode):
    """(D,) float64, the formulas of neighbour_image_kernel.  kind 0: Pearson correlation from the moments ``num``; kind 1:
    cov (ddof 1) of the ``num`` movie over sqrt(var var) (ddof 0) of the movie whose moments are ``den`` (rows 0 and 1).
    mode 0: the running maximum over the existing neighbours from 0 on, with Python's ``max``: a value replaces the
    maximum unless ``maximum > value`` is true, so a NaN replaces it and is itself replaced by the next neighbour.
    mode 1: the mean over the existing neighbours; no neighbour at all gives 0 / 0."""
    num = np.asarray(num, dtype=np.float64)
    D, n = d1 * d2, np.float64(T)
    q, exists = neighbour_index(d1, d2)
    dsum, dsq = (num[0], num[1]) if kind == 0 else (np.asarray(den, dtype=np.float64)[0], np.asarray(den, dtype=np.float64)[1])
    with np.errstate(all="ignore"):
        ss = dsq - dsum * dsum / n
        best, total, count = np.zeros(D), np.zeros(D), np.zeros(D)
        for k in range(8):
            cross = num[2 + k] - num[0] * num[0][q[k]] / n
            if kind == 0:
                val = cross / np.sqrt(ss * ss[q[k]])
            else:
                val = (cross / (n - 1.0)) / np.sqrt((ss / n) * (ss[q[k]] / n))
            e = exists[k]
            total = np.where(e, total + val, total)
            best = np.where(e & ~(best > val), val, best)
            count = count + e
        return best if mode == 0 else total / count


def lag_image(mom, n):
    """(D,) float64, the formula of lag_image_kernel on the (5, D) lag moments of n pairs."""
    sx, sxx, sy, syy, sxy = np.asarray(mom, dtype=np.float64)
    n = np.float64(n)
    with np.errstate(all="ignore"):
        return (sxy - sx * sy / n) / (np.sqrt(sxx - sx * sx / n) * np.sqrt(syy - sy * sy / n))


def csr_rows_spmm(indptr, indices, data, rows, B, ncols, absolute=False):
    """(n_sel, ncols): out[p][f] = sum over the nonzeros i of CSR row rows[p] (rows None: every row in order) of
    data[i] * B[indices[i]][f]."""
    data, B = _wide(data, B)
    if absolute:
        data, B = np.abs(data.astype(np.float64)), np.abs(B.astype(np.float64))
    rows = np.arange(len(indptr) - 1) if rows is None else np.asarray(rows)
    out = np.zeros((len(rows), ncols), dtype=data.dtype)
    for p, row in enumerate(rows):
        for i in range(int(indptr[row]), int(indptr[row + 1])):
            out[p] += data[i] * B[indices[i], :ncols]
    return out


def transpose_affine(src, scale=None, shift=None):
    """(cols, rows): dst[c][r] = src[r][c] * scale[r] + shift[r]; a missing scale is 1, a missing shift 0."""
    args = [np.asarray(src)] + [np.asarray(v) for v in (scale, shift) if v is not None]
    wide = _wide(*args)
    out = wide.pop(0)
    if scale is not None:
        out = out * wide.pop(0)[:, None]
    if shift is not None:
        out = out + wide.pop(0)[:, None]
    return np.ascontiguousarray(out.T)
