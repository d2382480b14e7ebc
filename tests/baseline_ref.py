"""NumPy emulations of the rolling-baseline kernels (csrc/baseline.hip), operation by operation in float32: the bin chains
of pmd_bin_means, the sliding extrema of pmd_sliding_extremum (two forms: the padded window view that is pinned against
scipy on the CPU, and a shift loop with fmin / fmax that also defines the NaN cases), the bin centres, the interpolation
and the three outputs of pmd_baseline_apply, and the whole of rolling_baseline / dff_movie on a (T, N) float32 movie.
Written independently of localmd_amd.baseline: the tests compare the two."""
import numpy as np

f32 = np.float32


def half_of(window, b):
    """The smallest h >= 0 with (2 h + 1) b >= window, by search."""
    h = 0
    while (2 * h + 1) * b < window:
        h += 1
    return h


def bin_chain(y, b):
    """(ceil(n / b), N) float32: per bin of b frames of the (n, N) block the fp32 chain over its frames in ascending
    order starting from the first frame's value, divided by the frame count; b == 1: the values themselves."""
    y = np.asarray(y).astype(f32)
    if b == 1:
        return y.copy()
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, len(y), b):
            blk = y[s:s + b]
            acc = blk[0].copy()
            for k in range(1, len(blk)):
                acc = (acc + blk[k]).astype(f32)
            out.append((acc / f32(len(blk))).astype(f32))
    return np.stack(out)


def movie_knots(y, b, block=1024):
    """bin_chain over a (T, N) movie: the same thing, as b divides the block; kept blockwise as the device does it."""
    return np.concatenate([bin_chain(y[c0:c0 + block], b) for c0 in range(0, len(y), block)])


def sliding_view(x, h, is_max):
    """The sliding extremum of the NaN-free (n, N) array x over [j - h, j + h], cut at both ends: the window view of x
    padded with +inf (-inf for the maximum)."""
    x = np.asarray(x, dtype=f32)
    pad = np.full((h,) + x.shape[1:], -np.inf if is_max else np.inf, f32)
    v = np.lib.stride_tricks.sliding_window_view(np.concatenate([pad, x, pad]), 2 * h + 1, axis=0)
    return (v.max(axis=-1) if is_max else v.min(axis=-1)).astype(f32)


def sliding(x, h, is_max):
    """The same by shifts, with fmin / fmax: a NaN is dropped unless the whole (cut) window is NaN."""
    x = np.asarray(x, dtype=f32)
    n = len(x)
    op = np.fmax if is_max else np.fmin
    out = x.copy()
    for s in range(1, min(h, n - 1) + 1):
        out[s:] = op(out[s:], x[:-s])
        out[:-s] = op(out[:-s], x[s:])
    return out


def filtered(k, h, method):
    lo = sliding(k, h, False)
    return sliding(lo, h, True) if method == "maximin" else lo


def centres(T, b):
    """The bin centres as Python floats: bin j has n_j = min(b, T - j b) frames and the centre j b + (n_j - 1) / 2."""
    return [j * b + (min(b, T - j * b) - 1) / 2.0 for j in range(-(-T // b))]


def baseline_frames(K, T, b, t0, t1):
    """(t1 - t0, N) float32: the baseline at frames t0 .. t1 from the knots K, frame by frame."""
    K = np.asarray(K, dtype=f32)
    c = centres(T, b)
    out = np.empty((t1 - t0,) + K.shape[1:], f32)
    j = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(t0, t1):
            if t <= c[0]:
                out[t - t0] = K[0]
                continue
            if t >= c[-1]:
                out[t - t0] = K[-1]
                continue
            while not (c[j] <= t < c[j + 1]):
                j = j + 1 if c[j + 1] <= t else j - 1
            if t == c[j]:
                out[t - t0] = K[j]
                continue
            w = f32(f32(t - c[j]) / f32(c[j + 1] - c[j]))
            d = (K[j + 1] - K[j]).astype(f32)
            out[t - t0] = (K[j] + (w * d).astype(f32)).astype(f32)
    return out


def outputs(x, F0, output, min_baseline=0.0):
    x, F0 = np.asarray(x).astype(f32), np.asarray(F0, dtype=f32)
    if output == "baseline":
        return F0.copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = (x - F0).astype(f32)
        if output == "detrended":
            return r
        q = (r / F0).astype(f32)
    return np.where(F0 > f32(min_baseline), q, f32(0)).astype(f32)


def dff(y, b, h, method, output, min_baseline=0.0):
    """(knots, output frames) of the whole pipeline on the (T, N) movie y."""
    T = len(y)
    K = filtered(movie_knots(y, b), h, method)
    return K, outputs(y, baseline_frames(K, T, b, 0, T), output, min_baseline)


def same_bits(a, b):
    """a and b (float32) agree bit for bit, except that any NaN matches any NaN (the payload and sign of a NaN that
    arithmetic produced differ between processors)."""
    a, b = np.ascontiguousarray(a, dtype=f32), np.ascontiguousarray(b, dtype=f32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
