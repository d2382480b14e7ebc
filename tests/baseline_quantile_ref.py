"""NumPy references for the percentile baseline (pmd_sliding_quantile, csrc/baseline.hip, and method="percentile" of
localmd_amd.baseline): the sliding order statistic as a window sort on the keys of quantiles.float_keys, the rank rule,
the filtered knots and the whole dF/F through the emulations of tests/baseline_ref.py; and an operation-by-operation
emulation of the kernel's incremental rule (bisection for the first output of a slice, then one member out, one in, and
a step to the neighbouring distinct key), which the host tests compare with the window sort."""
import math

import numpy as np

from localmd_amd.quantiles import float_keys, key_floats
from tests import baseline_ref as R

f32 = np.float32


def window_rows(n, h, j):
    """The 2 h + 1 row indices of the window of output j: j - h .. j + h clamped into 0 .. n - 1 (edges replicated)."""
    return np.clip(np.arange(j - h, j + h + 1), 0, n - 1)


def sliding_ranks(x, h, ranks):
    """{k: (n, N) float32} for the ranks k: per output j the window X[clamp(j + i)], i = -h .. h, as keys, sorted, the
    member at position k, back as a float (a NaN comes out as key_floats(0xFFFFFFFF))."""
    x = np.asarray(x, dtype=f32)
    n = len(x)
    keys = float_keys(x).reshape(x.shape)
    out = {int(k): np.empty(x.shape, np.uint32) for k in ranks}
    for j in range(n):
        s = np.sort(keys[window_rows(n, h, j)], axis=0)
        for k in out:
            out[k][j] = s[k]
    return {k: key_floats(v).reshape(x.shape) for k, v in out.items()}


def sliding_rank(x, h, k):
    return sliding_ranks(x, h, [k])[int(k)]


def weighted_rank(x, h, k):
    """sliding_rank without building the window, for any h: the rows a window really holds with the number of times it
    holds them (members), sorted by key, and the first whose cumulative count exceeds k."""
    x = np.asarray(x, dtype=f32)
    n = len(x)
    keys = float_keys(x).reshape(x.shape)
    out = np.empty(x.shape, np.uint32)
    for j in range(n):
        rows, mult = members(n, h, j)
        for c in range(x.shape[1]):
            order = np.argsort(keys[rows, c], kind="stable")
            at = int(np.searchsorted(np.cumsum(mult[order]), k, side="right"))
            out[j, c] = keys[rows[order[at]], c]
    return key_floats(out).reshape(x.shape)


def rank_of(h, q):
    """min(W - 1, floor(q W)) with W = 2 h + 1, in float64."""
    W = 2 * h + 1
    return min(W - 1, int(math.floor(float(q) * float(W))))


def filtered_percentile(knots, h, q):
    return sliding_rank(knots, h, rank_of(h, q))


def dff(y, b, h, q, output, min_baseline=0.0):
    """(knots, output frames) of rolling_baseline / dff_movie with method="percentile" on the (T, N) movie y."""
    T = len(y)
    K = filtered_percentile(R.movie_knots(y, b), h, q)
    return K, R.outputs(y, R.baseline_frames(K, T, b, 0, T), output, min_baseline)


# ---- test series -----------------------------------------------------------------------------------------------------
SERIES_KINDS = ("gauss", "ties", "constant", "rising", "falling", "zeros", "denormal", "inf", "nan_short", "nan_window",
                "nan_long", "nan_all")


def series(rng, n, N, h, shift=0):
    """(n, N) float32 whose column c is of kind SERIES_KINDS[(c + shift) % 12]: Gaussians; integers in -3 .. 3 (ties);
    a constant; strictly rising and falling ramps (the answer moves at every step); -0 and +0 mixed with +-1 (the bits
    decide); denormals of both signs with zeros; Gaussians with +-inf; integers with a NaN run shorter than, equal to
    and longer than W = 2 h + 1; all NaN."""
    W = 2 * h + 1
    x = np.empty((n, N), f32)
    t = np.arange(n)
    for c in range(N):
        kind = SERIES_KINDS[(c + shift) % len(SERIES_KINDS)]
        at = int(rng.integers(0, n))
        if kind == "gauss":
            col = rng.standard_normal(n)
        elif kind == "constant":
            col = np.full(n, 2.5)
        elif kind == "rising":
            col = -3.0 + 0.25 * t
        elif kind == "falling":
            col = 7.0 - 0.5 * t
        elif kind == "zeros":
            col = rng.choice(np.array([-1.0, -0.0, 0.0, 1.0]), n)
        elif kind == "denormal":
            col = rng.integers(-3, 4, n) * np.float64(1e-45) * rng.choice(np.array([1.0, 1000.0]), n)
            col = np.where(rng.random(n) < 0.2, -0.0, col)
        elif kind == "inf":
            col = rng.standard_normal(n)
            col[rng.random(n) < 0.15] = np.inf
            col[rng.random(n) < 0.15] = -np.inf
        elif kind == "nan_all":
            col = np.full(n, np.nan)
        else:
            col = rng.integers(-3, 4, n).astype(np.float64)
            if kind != "ties":
                run = {"nan_short": max(1, h), "nan_window": W, "nan_long": W + 2}[kind]
                col[at:at + run] = np.nan
        x[:, c] = col.astype(f32)
    return x


# ---- the kernel's rule, one column at a time -------------------------------------------------------------------------
def members(n, h, j):
    """(rows, multiplicities) of a scan of the window of output j: the rows it really holds once each, then row 0 and
    row n - 1 again with the number of their replicated copies."""
    lo, hi = max(j - h, 0), min(j + h, n - 1)
    rows, mult = list(range(lo, hi + 1)), [1] * (hi - lo + 1)
    m0, m1 = max(h - j, 0), max(j + h - (n - 1), 0)
    if m0:
        rows.append(0)
        mult.append(m0)
    if m1:
        rows.append(n - 1)
        mult.append(m1)
    return np.array(rows), np.array(mult, dtype=np.int64)


def emulate_slice(keys, h, rank, j0, j1, stats=None):
    """The keys pmd_sliding_quantile writes for the outputs j0 .. j1 of one column (``keys``: its n uint32 keys) when a
    wave starts its slice at j0.  ``stats`` (a dict) counts scans and element visits."""
    keys = np.asarray(keys, dtype=np.uint32).astype(np.int64)
    n = len(keys)
    W = 2 * h + 1
    assert 0 <= rank < W
    visits = 0
    rows, mult = members(n, h, j0)
    assert mult.sum() == W and len(rows) <= min(W, n) + 2
    k = keys[rows]
    a = 0
    for b in range(31, -1, -1):                               # the smallest a with #{key <= a} > rank
        probe = a | ((1 << b) - 1)
        if mult[k <= probe].sum() <= rank:
            a |= 1 << b
        visits += len(rows)
    cl, ce = int(mult[k < a].sum()), int(mult[k == a].sum())
    visits += len(rows)
    assert ce > 0 and cl <= rank < cl + ce
    out = [a]
    scans = 33
    for j in range(j0 + 1, j1):
        ko, ki = keys[min(max(j - 1 - h, 0), n - 1)], keys[min(j + h, n - 1)]
        cl += int(ki < a) - int(ko < a)
        ce += int(ki == a) - int(ko == a)
        assert cl >= 0 and ce >= 0
        if rank < cl or rank - cl >= ce:
            rows, mult = members(n, h, j)
            assert mult.sum() == W
            k = keys[rows]
            scans += 1
            visits += len(rows)
            if rank < cl:                                     # down: the largest key below a, with its count
                assert cl == rank + 1
                lo = k[k < a].max()
                nlo = int(mult[k == lo].sum())
                a, ce, cl = int(lo), nlo, cl - nlo
            else:                                             # up: the smallest key above a, with its count
                assert cl + ce == rank
                hi = k[k > a].min()
                cl, a, ce = cl + ce, int(hi), int(mult[k == hi].sum())
            assert cl <= rank < cl + ce
        out.append(a)
    if stats is not None:
        stats["scans"] = stats.get("scans", 0) + scans
        stats["visits"] = stats.get("visits", 0) + visits
    return np.array(out, dtype=np.uint32)


def emulate(x, h, rank, S, offset=0, stats=None):
    """The (n,) float32 column pmd_sliding_quantile writes for the column x with slices of S outputs; ``offset`` < S
    shortens the first slice, so that every output can be made the first of a slice."""
    keys = float_keys(np.asarray(x, dtype=f32)).reshape(-1)
    n = len(keys)
    cuts = [0] + list(range(offset if offset else S, n, S)) + [n]
    parts = [emulate_slice(keys, h, rank, a, b, stats) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    return key_floats(np.concatenate(parts))
