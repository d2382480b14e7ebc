"""
Inputs and float64 restatements shared by the tests of the first temporal window of the tile stage (test infrastructure
only): tests/test_tile_stage_ref.py proves on the CPU, from the oracles alone, that the inputs are admissible;
tests/test_gpu_tile_kernels_wide.py, tests/test_gpu_tile_stage.py and tests/test_gpu_tile_degenerate.py run the device on them.

Two parts:
  - the Cholesky whitening of the 64-row path (small_chol_kernel): its inputs and the pivot rule restated in NumPy;
  - planted movies for pmd_tiles_decompose, the float64 / fp32 oracles of every tile (oracle.pmd_oracle.single_block_md),
    the separation criteria and the error measure K; the family of degenerate tiles (DEGENERATE, KINDS);
  - the device call of pmd_tiles_decompose with its guard tiles (device_run) and the exact check of its decisions.
"""
import contextlib
import functools
import zlib

import numpy as np

from localmd_amd import grid
from oracle import pmd_oracle as O, philox

# ------------------------------------------------------------------------------------------------------------------
# Cholesky whitening
# ------------------------------------------------------------------------------------------------------------------
CHOL_ORDERS = [1, 7, 50, 64]
CHOL_TOL = 1e-10
# exact scalings of the four tiles: the pivot rule is relative to the largest diagonal entry, so a dead pivot of tile 2 is far
# above tol in absolute terms and the live pivots of tiles 1 and 3 are far below it
CHOL_SCALES = [1.0, 2.0 ** -60, 2.0 ** 40, 2.0 ** -70]


def chol_dead_rows(n):
    """Rows of a deficient tile of order n that depend on earlier ones: row 3 and the last row are combinations of the
    rows before them and one row is zero (order 1: the only row is zero)."""
    if n < 7:
        return [0]
    return sorted({3, (2 * n) // 3, n - 1})


@functools.lru_cache(maxsize=None)
def chol_inputs(n):
    """(mats, dead): four n x n Gram matrices M = A A^T of integer-valued A (so M and the dependencies are exact in
    float64) and, per tile, the rows that must come out dead.  Tiles 0 and 1 have full rank, the rows of tile 1 scaled over 1.2
    decades (cond(M) <= 1e4); tiles 2 and 3 are deficient.  Tile b is scaled by CHOL_SCALES[b], a power of two."""
    rng = np.random.default_rng(1000 + n)
    mats, dead = [], []
    for b in range(4):
        A = rng.integers(-8, 9, size=(n, 600)).astype(np.float64)
        if b < 2:
            if b == 1:
                A *= 2.0 ** -np.round(4.0 * np.arange(n) / max(n - 1, 1))[:, None]   # powers of two: M stays exact
            dd = []
        else:
            dd = chol_dead_rows(n)
            if n >= 7:
                zero = (2 * n) // 3
                A[3] = 2 * A[0] - A[1] + 3 * A[2]
                A[zero] = 0
                A[n - 1] = A[: n - 1][rng.choice(n - 1, 4, replace=False)].sum(axis=0) if b == 3 else A[1] - A[n - 2]
            else:
                A[0] = 0
        mats.append((A @ A.T) * CHOL_SCALES[b])
        dead.append(dd)
    return mats, dead


def antisymmetric_split(mats, width, rng):
    """G[tile][2][width][width]: slices 0.25 M + A and 0.75 M - A with A antisymmetric, no larger than M's entries; the
    symmetrised slice sum is M.  Outside the leading block the slices hold NaN (never to be read)."""
    n = mats[0].shape[0]
    G = np.full((len(mats), 2, width, width), np.nan)
    for b, M in enumerate(mats):
        m = np.abs(M).mean()
        A = rng.standard_normal((n, n)) * min(m, np.sqrt(m))
        A = A - A.T
        G[b, 0, :n, :n] = 0.25 * M + A
        G[b, 1, :n, :n] = 0.75 * M - A
    return G


def chol_whiten_ref(G, n, tol):
    """small_chol_kernel restated: G (slices, w, w); the leading n x n block of the symmetrised slice sum is factored
    M = R^T R by a right-looking Cholesky in the natural order; a pivot <= tol * max diagonal marks a dead row (unit
    pivot, zero row, no update).  Returns (N = R^-1 with the dead columns zeroed, pivots, dead mask, max diagonal)."""
    M = np.zeros((n, n))
    for k in range(G.shape[0]):
        M += G[k, :n, :n] + G[k, :n, :n].T
    M *= 0.5
    dmax = max(0.0, float(np.max(np.diag(M))))
    R = np.triu(M)
    piv = np.zeros(n)
    dead = np.zeros(n, dtype=bool)
    for k in range(n):
        piv[k] = R[k, k]
        dead[k] = not (piv[k] > tol * dmax)
        if dead[k]:
            R[k, k:] = 0.0
            R[k, k] = 1.0
            continue
        R[k, k:] /= np.sqrt(piv[k])
        for i in range(k + 1, n):
            R[i, i:] -= R[k, i] * R[k, i:]
    N = np.linalg.inv(R)
    N[:, dead] = 0.0
    return N, piv, dead, dmax


# ------------------------------------------------------------------------------------------------------------------
# pmd_tiles_decompose: planted movies and their oracles
# ------------------------------------------------------------------------------------------------------------------
KNIFE_EDGE = 2e-3
SEED = 31
PASS_ALL = (1024.0, 1024.0)
MAX_FAILS = [1, 2, 3]
N_SMOOTH = 6

# name: movie (field of view, frames, planted components, amplitude ratio, noise), block, temporal_avg_factor a, pooling
# factor, max_components r, the case's own (spatial, temporal) thresholds
MOVIES = {
    "m30": dict(fov=(30, 30), T=400, K=60, ratio=0.95, noise=0.01),
    "m30w": dict(fov=(30, 30), T=400, K=88, ratio=0.96, noise=0.01),
    "m30x": dict(fov=(30, 30), T=800, K=165, ratio=0.975, noise=0.01),
    "m40": dict(fov=(40, 40), T=400, K=53, ratio=0.95, noise=0.01),
    "m30s": dict(fov=(30, 30), T=100, K=22, ratio=0.9, noise=0.01),
    "m15": dict(fov=(15, 15), T=400, K=100, ratio=0.96, noise=0.01),
    "many": dict(fov=(72, 72), T=96, K=12, ratio=0.7, noise=0.01),
}
CASES = {
    "A": dict(movie="m30", block=(20, 20), a=4, pool=2, r=54, thr=(0.877924, 0.890593)),
    "B": dict(movie="m30", block=(20, 20), a=4, pool=2, r=55, thr=(0.877922, 0.89059)),
    "C": dict(movie="m30w", block=(20, 20), a=4, pool=2, r=80, thr=(1.071368, 1.562973)),
    "D": dict(movie="m30x", block=(20, 20), a=4, pool=1, r=150, thr=(0.716916, 1.205644)),
    "E": dict(movie="m40", block=(30, 30), a=4, pool=1, r=48, thr=(0.821566, 0.690261)),
    "F1w": dict(movie="m30s", block=(20, 20), a=10, pool=2, r=80, thr=(0.703943, 0.934488)),
    "F1n": dict(movie="m30s", block=(20, 20), a=10, pool=2, r=20, thr=(0.703943, 0.934488)),
    "F2p": dict(movie="m15", block=(10, 10), a=4, pool=2, r=95, thr=(0.791795, 1.187666)),
    "F2q": dict(movie="m15", block=(10, 10), a=4, pool=1, r=95, thr=(0.82439, 1.200111)),
    "many": dict(movie="many", block=(8, 8), a=4, pool=1, r=6, thr=(1.204495, 0.740683)),
}
# required numbers of separated components per tile: (all, at index >= 64, at index >= 128)
MIN_SEPARATED = {"A": (30, 0, 0), "B": (30, 0, 0), "C": (30, 5, 0), "D": (30, 5, 5), "E": (30, 0, 0)}
MANY_CALLS = (4095, 4096)
MANY_SAMPLE = 64

# Degenerate tiles: constant, dead and low-rank content next to ordinary tiles in one launch.  The tiles are disjoint, tile t is
# rows [t d, (t + 1) d) of one pixel-major matrix (pixel q = i + b1 j of the tile).  The first four kinds hold small integers
# (every value, product and rank exact in fp32); RHO is their rank.  "live" is an ordinary planted tile (planted() with K
# components), "deadrows" one with image rows 4-5 and image column 0 zeroed.
KINDS = ("zero", "low3", "rank1", "sparse2", "deadrows", "live", "live")
RHO = {"zero": 0, "low3": 3, "rank1": 1, "sparse2": 2}
LIVE_TILES = (5, 6)
# The spatial threshold stands above the statistic of a single live pixel (20 / 9: "sparse2" has two such pixels), the
# temporal one in the widest gap of the float64 oracle's temporal statistics over all tiles (Zn: 0.53 | 1.11, Zw: 0.97 | 1.31):
# the null directions fail on the temporal statistic.
DEGENERATE = {
    "Zn": dict(block=(10, 10), T=96, a=4, pool=2, r=6, K=12, ratio=0.7, noise=0.01, thr=(2.5, 0.76)),
    "Zw": dict(block=(10, 10), T=400, a=4, pool=1, r=60, K=100, ratio=0.96, noise=0.01, thr=(2.5, 1.12)),
}
SCALES = (2.0 ** 24, 2.0 ** -24)


def _sinusoid(T, amp, cycles, phase):
    return np.round(amp * np.sin(2.0 * np.pi * cycles * np.arange(T) / T + phase))


def _bump(b1, b2, amp, ci, cj, width):
    i, j = np.meshgrid(np.arange(b1), np.arange(b2), indexing="ij")
    return np.round(amp * np.exp(-((i - ci) ** 2 + (j - cj) ** 2) / (2.0 * width ** 2)))


@functools.lru_cache(maxsize=None)
def degenerate_rows(name):
    """(len(KINDS) d, T) float32: the tiles of KINDS one behind the other."""
    c = DEGENERATE[name]
    (b1, b2), T = c["block"], c["T"]
    d = b1 * b2
    out = np.zeros((len(KINDS), d, T), dtype=np.float64)
    for t, kind in enumerate(KINDS):
        if kind == "low3":
            F = np.stack([_bump(b1, b2, 9, 3, 3, 2.0), _bump(b1, b2, 9, 6, 7, 2.5), np.ones((b1, b2))]).reshape((3, d), order="F")
            B = np.stack([_sinusoid(T, 12, 1, 0.0), _sinusoid(T, 12, 2, np.pi / 2), _sinusoid(T, 12, 3, 0.5)])
            out[t] = F.T @ B
        elif kind == "rank1":
            out[t] = _sinusoid(T, 40, 2, 0.3)[None, :]
        elif kind == "sparse2":
            out[t, 2 + b1 * 3] = _sinusoid(T, 50, 1.5, 0.0)
            out[t, 7 + b1 * 6] = _sinusoid(T, 30, 2.5, np.pi / 2)
        elif kind in ("deadrows", "live"):
            rng = np.random.default_rng(zlib.crc32(f"tile-stage/{name}/{t}".encode()))
            blk = planted((b1, b2), T, c["K"], c["ratio"], c["noise"], rng)
            if kind == "deadrows":
                blk[4:6, :, :] = 0
                blk[:, 0, :] = 0
            out[t] = blk.reshape((d, T), order="F")
    assert np.abs(out[:4]).max() < 2 ** 12 and np.array_equal(out[:4], np.round(out[:4]))
    return np.ascontiguousarray(out.reshape(len(KINDS) * d, T), dtype=np.float32)


def pooled_binned(name, t):
    """The pooled, temporally binned block of tile t as single_block_md forms it, float64 (pooled pixels, bins)."""
    c = cfg(name)
    block = tile_block(name, t).astype(np.float64)
    with O.arbiter_precision():
        pooled = O.downsample_average_pooling(block, c["pool"])
    return np.mean(np.reshape(pooled, (pooled.shape[0] * pooled.shape[1], c["a"], block.shape[2] // c["a"]), order="F"), axis=1)


def oracle_rank(ref, thr, max_fail):
    """Components that filter_by_failures keeps from the statistics of an oracle tile (a NaN statistic fails)."""
    with np.errstate(invalid="ignore"):
        good = (ref.sp < np.float32(thr[0])) & (ref.tp < np.float32(thr[1]))
    return int(O.filter_by_failures(good.copy(), max_fail).sum())


def cfg(name):
    """The entry of CASES or of DEGENERATE (below) under that name."""
    return CASES[name] if name in CASES else DEGENERATE[name]


def case_dims(name):
    c = cfg(name)
    if name in DEGENERATE:
        return (c["block"][0], c["block"][1] * len(KINDS)), c["block"], c["T"]
    m = MOVIES[c["movie"]]
    return m["fov"], c["block"], m["T"]


def r_eff(name):
    """min(r, bins, pooled pixels): the components that exist (decomposition.py:59-73: u_final[:, :rank] of a sketch
    of r + 10 columns)."""
    c = cfg(name)
    (_, _), (b1, b2), T = case_dims(name)
    pooled = -(-b1 // c["pool"]) * -(-b2 // c["pool"])
    return min(c["r"], T // c["a"], pooled)


def planted(fov, T, K, ratio, noise, rng):
    """X = F diag(amp) B sqrt(D T) + noise N(0, 1), float32 (d1, d2, T): F unit-norm fields and B unit-norm traces, the
    first six smooth (Gaussian filtered) except the second field, which is white like every later one; amp_k = ratio^k."""
    from scipy.ndimage import gaussian_filter, gaussian_filter1d

    d1, d2 = fov
    D = d1 * d2
    F = rng.standard_normal((K, d1, d2))
    B = rng.standard_normal((K, T))
    for k in range(min(N_SMOOTH, K)):
        if k != 1:
            F[k] = gaussian_filter(F[k], 3.0, mode="reflect")
        B[k] = gaussian_filter1d(B[k], 8.0, mode="reflect")
    F = F.reshape(K, D)
    F /= np.linalg.norm(F, axis=1, keepdims=True)
    B /= np.linalg.norm(B, axis=1, keepdims=True)
    amp = ratio ** np.arange(K)
    X = (F.T * amp) @ B * np.sqrt(D * T) + noise * rng.standard_normal((D, T))
    return np.ascontiguousarray(X.reshape(d1, d2, T), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def planted_movie(movie):
    """The planted movie of MOVIES[movie] (see planted), float32 (d1, d2, T)."""
    m = MOVIES[movie]
    return planted(m["fov"], m["T"], m["K"], m["ratio"], m["noise"], np.random.default_rng(zlib.crc32(f"tile-stage/{movie}".encode())))


@functools.lru_cache(maxsize=None)
def tiles(name):
    """(pix (n, d) int32, origins (n, 2)): the driver's overlapping grid; the many-tiles case has an origin at every pixel
    offset 0 .. 64 of both dimensions (4225 tiles)."""
    fov, block, _ = case_dims(name)
    if name in DEGENERATE:
        d = block[0] * block[1]
        return np.arange(len(KINDS) * d, dtype=np.int32).reshape(len(KINDS), d), np.zeros((len(KINDS), 2), dtype=np.int64)
    if name == "many":
        it1 = it2 = list(range(fov[0] - block[0] + 1))
    else:
        it1, it2 = grid.tile_origins(fov, block)
    pix, origins = grid.tile_pixel_lists(fov, block, it1, it2)
    assert (pix[:, 1:] - pix[:, :-1] != 1).any()
    return pix, origins


@functools.lru_cache(maxsize=None)
def movie_rows(name):
    """The pixel-major matrix (D, T) float32 that the tile table of a case indexes."""
    if name in DEGENERATE:
        return degenerate_rows(name)
    fov, _, T = case_dims(name)
    return planted_movie(CASES[name]["movie"]).reshape(fov[0] * fov[1], T)


def omega_indices(name):
    """omega_index0 and omega_index_step as the driver forms them (t_lo * n_win + widx, n_win)."""
    n_win = 2 + len(name) % 3
    return 5 * n_win + 1, n_win


def omega_of_tile(src, name, t):
    c = cfg(name)
    _, _, T = case_dims(name)
    i0, step = omega_indices(name)
    return src.omega(philox.STREAM_TILE_OMEGA, i0 + t * step, T // c["a"], c["r"] + 10)


def tile_block(name, t):
    fov, (b1, b2), T = case_dims(name)
    if name in DEGENERATE:
        d = b1 * b2
        return degenerate_rows(name)[t * d:(t + 1) * d].reshape((b1, b2, T), order="F")
    k, j = tiles(name)[1][t]
    return planted_movie(CASES[name]["movie"])[k:k + b1, j:j + b2, :]


@contextlib.contextmanager
def lapack_precision(value):
    saved = O.LAPACK_PRECISION
    O.LAPACK_PRECISION = value
    try:
        yield
    finally:
        O.LAPACK_PRECISION = saved


MODES = ("f64", "f32", "f32s")   # the float64 arbiter, the fp32 oracle, the fp32 oracle with single-precision LAPACK


class TileRef:
    pass


def oracle_tile(name, t, omega, mode):
    """single_block_md of tile t.  u (d, r_eff), v (r_eff, T) = sigma V, the two statistics, and the two intermediate
    arrays the denoiser hooks see: v_ds (r_eff, T) and S = block_2d v_mat_basis^T (d, r_eff), and s_ds, the singular values
    of the pooled, binned block."""
    c = cfg(name)
    block = tile_block(name, t)
    seen = {}

    def temporal(v):
        seen["v_ds"] = np.array(v)
        return v

    def spatial(s):
        seen["S"] = np.array(s)
        return s

    def run():
        # (the singular values of the pooled, binned block: they condition the rows of v_ds)
        pooled = O.downsample_average_pooling(block.astype(O.F32, copy=False), c["pool"])
        binned = np.mean(np.reshape(pooled, (pooled.shape[0] * pooled.shape[1], c["a"], block.shape[2] // c["a"]), order="F"),
                         axis=1, dtype=O.F32)
        seen["s_ds"] = O.truncated_random_svd(binned, omega, c["r"])[1]
        return O.single_block_md(block, omega, c["r"], c["a"], c["pool"], 1.0, 1.0, spatial_denoiser=spatial,
                                 temporal_denoiser=temporal)

    if mode == "f64":
        with O.arbiter_precision():
            u, _, v, st = run()
    elif mode == "f32":
        with lapack_precision("double"):
            u, _, v, st = run()
    else:
        with lapack_precision("single"):
            u, _, v, st = run()
    out = TileRef()
    out.s_ds = np.asarray(seen["s_ds"], dtype=np.float64)
    out.u = u.reshape((-1, u.shape[2]), order="F")
    out.v = v
    out.sp, out.tp = np.asarray(st["spatial"]), np.asarray(st["temporal"])
    out.v_ds = seen["v_ds"]
    s = seen["S"]
    out.S = s.transpose(1, 2, 0).reshape((-1, s.shape[0]), order="F")
    return out


def separation(sig):
    """Relative gaps of a descending spectrum, which entries are strong (above 1e-3 of the first) and which separated (gap
    above 2e-2 and strong): the criteria of test_tiles_decompose_vs_oracle."""
    sig = np.asarray(sig, dtype=np.float64)
    strong = sig > 1e-3 * sig[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        gaps = np.minimum(np.abs(np.diff(sig, prepend=np.inf)), np.abs(np.diff(sig, append=0))) / sig
    return gaps, strong, (gaps > 2e-2) & strong


def vector_K(got, ref, sig, s0, sep, axis):
    """max over the separated components c of rel_err(got_c, ref_c) gap_c sig_c / s0 after sign alignment: the constant
    K of the bound K s0 / (gap_c sig_c).  axis 0: components are columns, 1: rows."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    gaps = separation(sig)[0]
    dots = np.sum(got * ref, axis=axis, keepdims=True)
    al = got * np.where(dots < 0, -1.0, 1.0)
    err = np.linalg.norm(al - ref, axis=axis) / np.maximum(np.linalg.norm(ref, axis=axis), 1e-300)
    k = err * gaps * sig / s0
    return float(np.max(k[sep])) if np.any(sep) else 0.0


def scalar_K(got, ref, sep):
    """max relative error over the separated components."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got[sep] - ref[sep]) / np.abs(ref[sep]))) if np.any(sep) else 0.0


def margin_ok(sp, tp, thr):
    """Every statistic farther than KNIFE_EDGE (relative) from its threshold."""
    m = np.minimum(np.abs(sp - thr[0]) / thr[0], np.abs(tp - thr[1]) / thr[1])
    return bool(np.all(m > KNIFE_EDGE))


def thresholds(name):
    """The case's own pair, rounded to fp32 (the device takes floats), and the pair that passes everything."""
    s, t = cfg(name)["thr"]
    return [(float(np.float32(s)), float(np.float32(t))), PASS_ALL]


def clearance(stats_list, thr):
    """Smallest relative distance of any statistic of any oracle to its threshold.  stats_list: [(sp, tp)]."""
    return min(float(np.min(np.abs(sp - thr[0]) / thr[0])) for sp, _ in stats_list), \
        min(float(np.min(np.abs(tp - thr[1]) / thr[1])) for _, tp in stats_list)


def decision_patterns(stats64, thr):
    """Which of "pass after a failure" and "cut by max_fail" the float64 oracle's decisions show over the tiles and
    max_fail in MAX_FAILS.  stats64: [(sp, tp)] per tile."""
    seen = set()
    for sp, tp in stats64:
        good = (sp < np.float32(thr[0])) & (tp < np.float32(thr[1]))
        for mf in MAX_FAILS:
            nk = int(O.filter_by_failures(good.copy(), mf).sum())
            if np.any(good[1:nk] & ~good[:nk - 1][:len(good[1:nk])]):
                seen.add("pass after a failure")
            if nk < len(good):
                seen.add("cut by max_fail")
    return seen


THR_RANGE = ((0.5, 1.38), (0.5, 2.3))   # between the smooth statistics and those of white fields / traces (1.41 / 2.45)
THR_CANDIDATES = 12


def _gap_middles(values, lo, hi):
    v = np.sort(np.asarray([x for x in values if lo < x < hi] + [lo, hi], dtype=np.float64))
    ratios = v[1:] / v[:-1]
    best = np.argsort(-ratios, kind="stable")[:THR_CANDIDATES]
    return [float(np.float32(np.sqrt(v[i] * v[i + 1]))) for i in best]


def best_thresholds(stats_all, stats64):
    """The (spatial, temporal) pair, each the fp32-rounded geometric middle of one of the THR_CANDIDATES widest empty
    intervals of the statistics inside THR_RANGE, with the largest smaller-of-the-two clearance among the pairs for
    which the float64 oracle's decisions show both patterns.  stats_all: [(sp, tp)] of the strong components of every
    oracle and tile; stats64: [(sp, tp)] of all components of the float64 oracle per tile.  Returns (pair, clearance)."""
    sp_all = np.concatenate([s for s, _ in stats_all])
    tp_all = np.concatenate([t for _, t in stats_all])
    best, best_c = None, -1.0
    for ts in _gap_middles(sp_all, *THR_RANGE[0]):
        for tt in _gap_middles(tp_all, *THR_RANGE[1]):
            c = min(clearance(stats_all, (ts, tt)))
            if c > best_c and len(decision_patterns(stats64, (ts, tt))) == 2:
                best, best_c = (ts, tt), c
    return best, best_c


@functools.lru_cache(maxsize=None)
def many_sample():
    """The tiles of the many-tiles case that are compared with the oracle: tiles 0, 4094, 4095 and further ones spread
    evenly over the grid, MANY_SAMPLE in all, each with at least 3 separated components in the float64 oracle (omegas of
    oracle.philox.PhiloxSource: the choice needs no device)."""
    src = philox.PhiloxSource(SEED)
    chosen = []
    cand = [0, 4094, 4095] + [int(x) for x in np.linspace(17, 4080, 110).astype(int)]
    for t in cand:
        if t in chosen:
            continue
        ref = oracle_tile("many", t, omega_of_tile(src, "many", t), "f64")
        if separation(np.linalg.norm(ref.v, axis=1))[2].sum() >= 3:
            chosen.append(t)
        if len(chosen) == MANY_SAMPLE:
            break
    return tuple(chosen)


def case_oracles(name, src, tile_ids=None, modes=MODES):
    """{tile: {mode: TileRef}} for the tiles of a case (all of them by default), omegas drawn from src."""
    ids = range(len(tiles(name)[1])) if tile_ids is None else tile_ids
    out = {}
    for t in ids:
        om = omega_of_tile(src, name, t)
        out[t] = {m: oracle_tile(name, t, om, m) for m in modes}
    return out


def threshold_stats(refs):
    """(stats_all, stats64) of best_thresholds / clearance from the result of case_oracles."""
    stats_all, stats64 = [], []
    for by_mode in refs.values():
        strong = separation(np.linalg.norm(by_mode["f64"].v, axis=1))[1]
        for m in MODES:
            stats_all.append((by_mode[m].sp[strong], by_mode[m].tp[strong]))
        stats64.append((by_mode["f64"].sp, by_mode["f64"].tp))
    return stats_all, stats64


def block_s0(name, t):
    """Largest singular value of the tile's block."""
    b = tile_block(name, t)
    return float(np.linalg.norm(b.reshape((b.shape[0] * b.shape[1], -1), order="F").astype(np.float64), 2))


# ------------------------------------------------------------------------------------------------------------------
# pmd_tiles_decompose on the device (used by the tests marked gpu only; torch is imported where it is needed)
# ------------------------------------------------------------------------------------------------------------------
def _t():
    import torch

    return torch


def P(t):
    from localmd_amd._lib import ptr

    return ptr(t)


def to_device(ctx, a, dtype=None):
    return _t().from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ctx.device)


def poisoned(ctx, shape, dtype):
    """A device array whose every byte is 0xFF (NaN in both float types, -1 as int32)."""
    torch = _t()
    x = torch.empty(shape, dtype=dtype, device=ctx.device)
    x.view(torch.uint8).fill_(0xFF)
    return x


def untouched(t):
    return bool((t.contiguous().view(_t().uint8) == 0xFF).all())


class Run:
    pass


def device_run(ctx, name, thr, max_fail, n_tiles=None, staged=False, download=True, scale=1.0, first_tile=0):
    """One pmd_tiles_decompose call as the driver makes it (staged: pmd_tiles_decompose_staged with stages 1, 2, 4 and
    the hook arrays read between the calls), on a workspace and outputs full of NaN bytes, a guard tile behind the last
    one of every output.  The call holds the tiles first_tile .. first_tile + n_tiles - 1 of the case with the sketch
    matrices they have in the call of all tiles; the movie is multiplied by scale (a power of two)."""
    import ctypes

    torch, lib = _t(), ctx.lib
    c = cfg(name)
    (d1, d2), (b1, b2), T = case_dims(name)
    a, r, D, d = c["a"], c["r"], d1 * d2, b1 * b2
    pix_all, _ = tiles(name)
    n = len(pix_all) - first_tile if n_tiles is None else n_tiles
    assert first_tile + n <= len(pix_all)
    pool_q, pool_idx, pool_w, _ = grid.pooling_maps((b1, b2), c["pool"])
    Pn = pool_q.shape[0]
    rp, dpad, ld = int(lib.pmd_tile_rpad(r)), int(lib.pmd_tile_dpad(d)), int(lib.pmd_time_ld(T))
    xf = torch.zeros((D, ld), dtype=torch.float32, device=ctx.device)
    xf[:, :T] = to_device(ctx, movie_rows(name) * np.float32(scale))
    out = Run()
    out.n, out.rp, out.d, out.T, out.re = n, rp, d, T, r_eff(name)
    out.ut = poisoned(ctx, (n + 1, rp, dpad), torch.float32)
    out.v = poisoned(ctx, (n + 1, rp, ld), torch.float32)
    out.stats = poisoned(ctx, (n + 1, rp, 2), torch.float32)
    out.good = poisoned(ctx, (n + 1, rp), torch.int32)
    out.keep = poisoned(ctx, (n + 1, rp), torch.int32)
    out.ranks = poisoned(ctx, (n + 1,), torch.int32)
    out.lam = poisoned(ctx, (n + 1, rp), torch.float64)
    nbytes = int(lib.pmd_tiles_workspace_bytes(n, b1, b2, Pn, r, a, T, ld, D))
    assert nbytes > 0
    ws = ctx.workspace(nbytes)
    ws.fill_(0xFF)
    i0, step = omega_indices(name)
    tables = [to_device(ctx, pix_all[first_tile:first_tile + n], np.int32), to_device(ctx, pool_q, np.int32),
              to_device(ctx, pool_idx, np.int32), to_device(ctx, pool_w, np.float32)]
    args = (P(xf), ld, D, T, P(tables[0]), n, b1, b2, P(tables[1]), pool_q.shape[1], Pn, P(tables[2]), P(tables[3]), r, a,
            float(thr[0]), float(thr[1]), max_fail, SEED, i0 + first_tile * step, step, P(out.ut), P(out.v), ld, P(out.stats),
            P(out.good), P(out.keep), P(out.ranks), P(out.lam), P(ws), ws.numel())
    if not staged:
        ctx.call("pmd_tiles_decompose", *args)
    else:
        off_v, off_s = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert lib.pmd_tiles_hook_offsets(n, b1, b2, Pn, r, a, T, ld, D, ctypes.byref(off_v), ctypes.byref(off_s)) == 0
        assert off_v.value + n * rp * ld * 4 <= nbytes and off_s.value + n * rp * dpad * 4 <= nbytes
        ctx.call("pmd_tiles_decompose_staged", *args, 1)
        ctx.sync()
        out.v_ds = ws[off_v.value:off_v.value + n * rp * ld * 4].view(torch.float32).view(n, rp, ld)[:, :out.re, :T].cpu().numpy()
        ctx.call("pmd_tiles_decompose_staged", *args, 2)
        ctx.sync()
        out.S = ws[off_s.value:off_s.value + n * rp * dpad * 4].view(torch.float32).view(n, rp, dpad)[:, :out.re, :d].cpu().numpy()
        ctx.call("pmd_tiles_decompose_staged", *args, 4)
    ctx.sync()
    # what must hold after every call, checked where the arrays are: the guard tiles, and zeros from r_eff on
    re = out.re
    for arr in (out.ut, out.v, out.stats, out.good, out.keep, out.ranks, out.lam):
        assert untouched(arr[n:n + 1]), "guard tile written"
    assert not bool((out.ut[:n, re:] != 0).any()), "rows of Ut from r_eff on"
    assert not bool((out.v[:n, re:, :T] != 0).any()), "rows of V from r_eff on"
    assert not bool((out.stats[:n, re:] != 0).any()), "rows of stats from r_eff on"
    assert not bool((out.good[:n, re:] != 0).any()) and not bool((out.keep[:n, re:] != 0).any())
    assert not bool((out.lam[:n, re:] != 0).any()), "lam_out from r_eff on"
    assert not bool((out.ut[:n, :, d:] != 0).any()), "padding of Ut"
    out.dev_ut, out.dev_v = out.ut, out.v
    out.stats, out.good, out.keep = out.stats[:n].cpu().numpy(), out.good[:n].cpu().numpy(), out.keep[:n].cpu().numpy()
    out.ranks, out.lam = out.ranks[:n].cpu().numpy(), out.lam[:n].cpu().numpy()
    if download:
        out.ut, out.v = out.ut[:n, :re, :d].cpu().numpy(), out.v[:n, :re, :T].cpu().numpy()
    else:
        out.ut = out.v = None
    return out


def check_decisions(name, run, thr, max_fail, patterns):
    """good, keep and ranks follow exactly from the statistics the device returned (no knife edge enters; a NaN statistic
    is a failure, as in the reference's comparison)."""
    re = run.re
    thr32 = (np.float32(thr[0]), np.float32(thr[1]))
    sp, tp = run.stats[:, :re, 0], run.stats[:, :re, 1]
    with np.errstate(invalid="ignore"):
        good = (sp < thr32[0]) & (tp < thr32[1])
    np.testing.assert_array_equal(run.good[:, :re], good.astype(np.int32), err_msg=f"{name} {thr} {max_fail}")
    for t in range(run.n):
        kept = O.filter_by_failures(good[t].copy(), max_fail)
        np.testing.assert_array_equal(run.keep[t, :re], kept.astype(np.int32), err_msg=f"{name} tile {t}")
        nk = int(kept.sum())
        assert run.ranks[t] == nk, (name, t, run.ranks[t], nk)
        if np.any(good[t, 1:nk] & ~good[t, :nk - 1][:len(good[t, 1:nk])]):
            patterns.add("pass after a failure")
        if nk < re:
            patterns.add("cut by max_fail")
