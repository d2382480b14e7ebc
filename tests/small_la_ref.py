"""Inputs, float64 references, restatements, bounds and shape tables for the tests of the tile stage's small dense algebra
and statistics: pmdk_small_qr, pmdk_small_eig, pmdk_roughness (csrc/small_la.hip) and pmdk_tile_pool_bin (csrc/prep.hip).
Test infrastructure only: NumPy, no GPU.  tests/test_small_la_ref.py checks this module on the host,
tests/test_gpu_tile_small_la.py walks its tables on the device.

u = 2^-24 (fp32) and U64 = 2^-53 are unit roundoffs.  gamma(k, u) = k u / (1 - k u) bounds the relative error of a value
that has been through k rounded operations (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1).

small_qr, derived bounds (fp64 storage).  The kernel holds the matrix in fp64, so its Q before the output rounding is that
of Householder QR in fp64: orthonormal to c P l U64 (below 1e-10 at the largest fp64-storage shape) and with
Y = Q R to the same order.  The output rounding gives q^ = q (1 + delta), |delta| <= u, entry by entry, hence
  orthonormality   |q^_i . q^_j - q_i . q_j| <= (2 u + u^2) sum_q |q_qi| |q_qj| <= 2 u (1 + u)   (Cauchy-Schwarz);
                   the tests allow (P + 2) u: the sharp 2 u, and P u for the fp64 part and whatever a reader of the
                   bound does not want to rest on Cauchy-Schwarz (sum_q |q_qi| |q_qj| <= P max|q|^2 <= P);
  projection       Y - Q^ Q^T Y = -(E Q^T + Q E^T) Y + O(u^2), |E| <= u |Q|; entry (q, c):
                   u sum_j |Q_qj| |R_jc| + u sum_j |Q_qj| (|Q|^T |y_c|)_j <= u |y_c|_2 (1 + sqrt(nref))
                   <= u sqrt(P) (1 + sqrt(nref)) max|Y|  (rows of Q have norm <= 1, || |Q| ||_2 <= sqrt(nref));
                   a column the dependence rule cuts (left^2 <= dep_tol |column|^2) leaves at most sqrt(dep_tol) |y_c|_2 of
                   Y outside span(Q): + sqrt(dep_tol) sqrt(P) max|Y|; + 64 P U64 sqrt(P) max|Y| for the fp64 part.
Both are capped by the figures the v0 test has always used (5e-6, 1e-4 max(max|Y|, 1)).  With fp32 storage every store
to the matrix rounds and no closed form holds; there the kernel is held to qr_restated below, FACTOR times its figure.
"""
from collections import namedtuple

import numpy as np

from tests import eig_ref, tile_gemm_ref, tile_stage_ref

U32 = 2.0 ** -24
U64 = 2.0 ** -53
FACTOR = 4.0                       # the project's factor for oracle ratios
SCALES = tile_stage_ref.SCALES     # power-of-two scales of the QR data (bitwise covariance)
PMD_ERR_UNSUPPORTED = -5


def gamma(k, u):
    return k * u / (1.0 - k * u)


# ---- small_qr --------------------------------------------------------------------------------------------------------
QR_SHAPES = [(1, 1), (1, 5), (7, 20), (20, 20), (25, 20), (64, 64), (100, 1),      # small edges
             (100, 60), (101, 60),                                                   # ldm = P | 1: even and odd P
             (313, 60), (314, 60),                                                   # the two sides of the storage switch
             (629, 64), (628, 64)]                                                   # the largest matrix that fits
QR_UNSUPPORTED = [(630, 64), (10, 65)]
QR_TILE_KINDS = ("well", "well", "graded", "rank5", "zero_tail", "constant")
QR_WELL = (0, 1)
QR_COND_MAX = 1e3
QR_ORTH_CAP = 5e-6
QR_PROJ_CAP = 1e-4
QR_TAIL_BYTES = (64 + 260) * 8 + 16     # tau[64], scratch[260] doubles and the alignment slack of small_qr_kernel


def qr_storage(P, l):
    """pmd_launch_small_qr restated: 'f64', 'f32' or None (PMD_ERR_UNSUPPORTED)"""
    if l > 64:
        return None
    ldm = P | 1
    if l * ldm * 8 + QR_TAIL_BYTES <= 150 * 1024:
        return "f64"
    if l * ldm * 4 + QR_TAIL_BYTES <= 160 * 1024:
        return "f32"
    return None


def qr_dep_tol(storage):
    return 1e-24 if storage == "f64" else 1e-12


def _orth(rng, n):
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return q


def qr_tiles(P, l, seed=None):
    """The six float32 P x l tiles of QR_TILE_KINDS.  A well-conditioned tile has singular values 1 .. 0.1 in its leading
    nref = min(P, l) columns (the ones that decide Q) and normal columns behind them."""
    rng = np.random.default_rng(1000 * P + l if seed is None else seed)
    nref = min(P, l)

    def well():
        lead = (np.linalg.qr(rng.standard_normal((P, nref)))[0] * np.linspace(1.0, 0.1, nref)) @ _orth(rng, nref)
        Y = rng.standard_normal((P, l)) / np.sqrt(P)
        Y[:, :nref] = lead
        return rng.uniform(1.0, 5.0) * Y

    out = []
    for kind in QR_TILE_KINDS:
        if kind == "well":
            Y = well()
        elif kind == "graded":
            Y = well() * np.geomspace(1.0, 1e-3, l)[rng.permutation(l)][None, :]
        elif kind == "rank5":
            k = min(5, nref)
            Y = rng.standard_normal((P, k)) @ rng.standard_normal((k, l))
        elif kind == "zero_tail":
            Y = well()
            Y[:, l - l // 2:] = 0
        else:
            Y = np.broadcast_to(rng.standard_normal((1, l)) + 2.0, (P, l))
        out.append(np.ascontiguousarray(Y, dtype=np.float32))
    return out


def qr_cond(Y):
    """cond_2 of the leading nref columns of Y, which decide Q (for P >= l: of Y)"""
    s = np.linalg.svd(Y[:, :min(Y.shape)].astype(np.float64), compute_uv=False)
    return float(s[0] / s[-1])


def qr_reference(Y):
    """Q of numpy.linalg.qr of the widened matrix: LAPACK's sign convention beta = -sign(alpha) norm, the kernel's"""
    return np.linalg.qr(Y.astype(np.float64))[0][:, :min(Y.shape)]


def qr_restated(Y, storage):
    """small_qr_kernel in NumPy with its rounding points: every store to M is rounded to the storage type, all arithmetic
    is float64, the dependence rule included.  Returns Q as the kernel writes it (float32, P x nref)."""
    st = np.float64 if storage == "f64" else np.float32
    P, l = Y.shape
    nref = min(P, l)
    M = Y.astype(st)
    f = lambda a: np.asarray(a, dtype=np.float64)
    tau = np.zeros(nref)
    cn = (f(M) ** 2).sum(axis=0)
    dep_tol = qr_dep_tol(storage)

    def reflect(k, last):
        """apply H(k) to columns k + 1 .. last - 1"""
        if tau[k] == 0.0 or k + 1 >= last:
            return
        v = f(M[k + 1:, k])
        w = tau[k] * (f(M[k, k + 1:last]) + v @ f(M[k + 1:, k + 1:last]))
        M[k + 1:, k + 1:last] = (f(M[k + 1:, k + 1:last]) - np.outer(v, w)).astype(st)
        M[k, k + 1:last] = (f(M[k, k + 1:last]) - w).astype(st)

    for k in range(nref):
        sigma = float((f(M[k + 1:, k]) ** 2).sum())
        alpha = float(M[k, k])
        t, scale, beta = 0.0, 0.0, alpha
        if sigma > 0.0 and alpha * alpha + sigma > dep_tol * cn[k]:
            nrm = np.sqrt(alpha * alpha + sigma)
            beta = -nrm if alpha >= 0.0 else nrm
            t = (beta - alpha) / beta
            scale = 1.0 / (alpha - beta)
        tau[k] = t
        M[k, k] = st(beta)
        M[k + 1:, k] = (f(M[k + 1:, k]) * scale).astype(st)
        reflect(k, l)
    for k in range(nref - 1, -1, -1):
        reflect(k, nref)
        col = -tau[k] * f(M[:, k])
        col[:k] = 0.0
        col[k] = 1.0 - tau[k]
        M[:, k] = col.astype(st)
    return f(M[:, :nref]).astype(np.float32)


def qr_figures(Q, Y, Q64=None):
    """(orthonormality, projection residual, distance to Q64) of a P x nref Q, max-abs in float64"""
    Q, Y = Q.astype(np.float64), Y.astype(np.float64)
    orth = float(np.abs(Q.T @ Q - np.eye(Q.shape[1])).max())
    proj = float(np.abs(Y - Q @ (Q.T @ Y)).max())
    dist = None if Q64 is None else float(np.abs(Q - Q64).max())
    return orth, proj, dist


def qr_orth_bound(P):
    return min(QR_ORTH_CAP, (P + 2) * U32)


def qr_proj_cap(Y):
    return QR_PROJ_CAP * max(float(np.abs(Y).max()), 1.0)


def qr_proj_bound(Y, storage="f64"):
    """module docstring; fp64 storage only"""
    P, l = Y.shape
    nref, ymax = min(P, l), float(np.abs(Y).max())
    derived = np.sqrt(P) * ymax * (U32 * (1.0 + np.sqrt(nref)) + np.sqrt(qr_dep_tol(storage)) + 64 * P * U64)
    return min(qr_proj_cap(Y), derived)


def qr_dist_bound(Q64, cond, P):
    """entrywise: output rounding + first-order forward error of Householder QR in fp64"""
    return U32 * np.abs(Q64) + 64 * P * U64 * cond


# ---- small_eig -------------------------------------------------------------------------------------------------------
EIG_ORDERS = [1, 2, 3, 4, 5, 31, 32, 33, 50, 63, 64]
EIG_SLICES = [1, 2, 4]
EIG_TOLS = [0.0, 1e-10]
EIG_SCALES = [1.0, 2.0 ** 80, 2.0 ** -80]
EIG_FAMILY = ("flat", "nulls", "decades")       # _eig_mats of test_gpu_tile_kernels_wide.py, tiles 0, 1, 2
EIG_KINDS = eig_ref.KINDS + EIG_FAMILY
EIG_GREY = (1e-12, 1e-8)          # a factor 100 on either side of tol lambda_max, tol = 1e-10


def eig_nnull(n):
    return min(5, n - 1)


def eig_mats(n):
    """One float64 n x n matrix per entry of EIG_KINDS"""
    mats = [eig_ref.make_sym(kind, n, 7 * n + i).astype(np.float64) for i, kind in enumerate(eig_ref.KINDS)]
    rng = np.random.default_rng(100 + n)
    for b in range(3):
        A = rng.standard_normal((n, 300)) * np.logspace(0, -4 if b else 0, n)[:, None]
        if b == 1 and eig_nnull(n):
            A[n - eig_nnull(n):] = 0
        mats.append(A @ A.T)
    return mats


def eig_slices(mats, slices, outside, seed):
    """G[tile][slices][64][64]: unequal shares of M plus antisymmetric parts (tile_stage_ref.antisymmetric_split; one
    slice: their sum; four: each of the two split again), `outside` everywhere but in the leading n x n block."""
    rng = np.random.default_rng(seed)
    n = mats[0].shape[0]
    G2 = tile_stage_ref.antisymmetric_split(mats, 64, rng)
    if slices == 1:
        G = G2.sum(axis=1, keepdims=True)                       # the antisymmetric parts cancel here ...
        for b, M in enumerate(mats):
            G[b, 0, :n, :n] += G2[b, 0, :n, :n] - 0.25 * M       # ... so one of them is added again: M + A
    elif slices == 2:
        G = G2
    else:
        G = np.full((len(mats), 4, 64, 64), np.nan)
        for b, M in enumerate(mats):
            m = np.abs(M).mean()
            B = rng.standard_normal((n, n)) * min(m, np.sqrt(m))
            B = B - B.T
            g0, g1 = G2[b, 0, :n, :n], G2[b, 1, :n, :n]
            for k, blk in enumerate((0.5 * g0 + B, 0.25 * g1 - B, 0.5 * g0 - B, 0.75 * g1 + B)):
                G[b, k, :n, :n] = blk
    mask = np.ones((64, 64), dtype=bool)
    mask[:n, :n] = False
    G[:, :, mask] = outside
    return G


def eig_matrix_of(G, n):
    """The matrix the kernels factor: 0.5 sum_k (g_k + g_k^T) of the leading blocks, summed in their order"""
    sm = np.zeros((G.shape[0], n, n))
    for k in range(G.shape[1]):
        blk = G[:, k, :n, :n]
        sm = sm + (blk + np.swapaxes(blk, 1, 2))
    return 0.5 * sm


def eig_decided(w):
    """No eigenvalue of the spectrum w sits where the null rule at tol = 1e-10 could go either way."""
    w = np.asarray(w, dtype=np.float64)
    top = w.max(initial=0.0)
    if top <= 0.0:
        return True
    return not np.any((w > EIG_GREY[0] * top) & (w < EIG_GREY[1] * top))


def eig_expected_keep(w, tol):
    """(keep, pinned) from a descending float64 reference spectrum.  keep: the rule on the reference.  pinned: where an
    eigenvalue that meets the mode-0 bound (rtol 1e-9, atol 1e-12 max|lambda|, asserted on the same input) cannot be on the
    other side of the threshold max(tol lambda_max, 0): it is further from it than twice that bound."""
    w = np.asarray(w, dtype=np.float64)
    amax = np.abs(w).max()
    thr = max(tol * w[0], 0.0)
    return (w > thr) & (w > 0.0), np.abs(w - thr) > 2.0 * (1e-9 * np.abs(w) + 1e-12 * amax) + 2e-9 * thr


def eig_keep_rule(lam, tol):
    """the epilogue's rule on a descending spectrum: kept iff lam > tol lam[0] and lam > 0"""
    lam = np.asarray(lam, dtype=np.float64)
    return (lam > tol * lam[..., :1]) & (lam > 0.0)


# ---- tile_pool_bin ---------------------------------------------------------------------------------------------------
# fov: the tiles are the grid's blocks of a field of view (the oracle's pooling can then be compared); None: n_tiles random
# pixel lists over n_rows pixel rows.  extra: added to the tight tile stride P ld_ab.
PoolCase = namedtuple("PoolCase", "name block pool a T fov n_rows n_tiles kind extra")
POOL_CASES = [
    PoolCase("v0", (20, 12), 2, 10, 230, (30, 26), None, None, "normal", 0),
    PoolCase("partial2", (15, 11), 2, 4, 103, (22, 17), None, None, "normal", 32),      # frames 100..102 are dropped
    PoolCase("partial3", (10, 10), 3, 1, 37, (14, 13), None, None, "normal", 32),
    PoolCase("pool1", (7, 5), 1, 10, 60, None, 61, 6, "normal", 32),
    PoolCase("a4_random_pix", (20, 12), 2, 4, 50, None, 300, 6, "normal", 64),
    PoolCase("exact", (20, 12), 2, 4, 64, (30, 26), None, None, "exact", 32),
    PoolCase("bins2100", (4, 3), 2, 1, 2100, None, 20, 6, "normal", 32),                # second trip of the bin loop
    PoolCase("rows_two_chunks", (3, 2), 2, 1, 12, None, 32768 + 70, 6, "normal", 32),   # second chunk of bin_average
    PoolCase("tiles_two_chunks", (2, 2), 2, 2, 8, None, 50, 32768 + 3, "normal", 32),   # second chunk of tile_pool
]


def pool_inputs(case):
    """dict: X float32 (n_rows, T) (the caller pads), pix (n_tiles, d) int32, pool_q, P, nbins, origins (or None)"""
    from localmd_amd import grid

    rng = np.random.default_rng(sum(map(ord, case.name)))
    b1, b2 = case.block
    pool_q, _, _, _ = grid.pooling_maps(case.block, case.pool)
    origins = None
    if case.fov is not None:
        it1, it2 = grid.tile_origins(case.fov, case.block)
        pix, origins = grid.tile_pixel_lists(case.fov, case.block, it1, it2)
        n_rows = case.fov[0] * case.fov[1]
    else:
        n_rows = case.n_rows
        pix = np.empty((case.n_tiles, b1 * b2), dtype=np.int32)
        for t in range(case.n_tiles):
            win = min(n_rows, max(b1 * b2, 64))              # even tiles from the first rows, odd ones from the last
            pix[t] = rng.permutation(win)[:b1 * b2] + (0 if t % 2 == 0 else n_rows - win)
    if case.kind == "exact":
        X = rng.integers(-7, 8, size=(n_rows, case.T)).astype(np.float32)
    else:
        X = (rng.standard_normal((n_rows, case.T)) * np.logspace(0, 2, n_rows)[rng.permutation(n_rows)][:, None]).astype(np.float32)
    return dict(X=X, pix=np.ascontiguousarray(pix, dtype=np.int32), pool_q=pool_q, P=pool_q.shape[0], nbins=case.T // case.a,
                origins=origins)


def pool_reference(X, pix, pool_q, a, nbins, tiles=None):
    """float64: (xbar, |x| bin means, abar, window means of the |x| bin means, window counts)"""
    x = X[:, :a * nbins].astype(np.float64).reshape(X.shape[0], nbins, a)
    xbar, xabs = x.mean(axis=2), np.abs(x).mean(axis=2)
    pix = pix if tiles is None else pix[tiles]
    member = pool_q >= 0
    cnt = member.sum(axis=1)
    abar = np.zeros((pix.shape[0], pool_q.shape[0], nbins))
    aabs = np.zeros_like(abar)
    for p in range(pool_q.shape[0]):
        rows = pix[:, pool_q[p][member[p]]]              # (tiles, cnt)
        abar[:, p] = xbar[rows].mean(axis=1)
        aabs[:, p] = xabs[rows].mean(axis=1)
    return xbar, xabs, abar, aabs, cnt


def pool_bounds(a, xabs, aabs, cnt):
    """Two fp32 chains.  xbar: a - 1 adds, the rounded 1 / a and the product: (a + 1) u mean|x|.  abar: on top of that cnt - 1
    adds, the rounded 1 / cnt and the product: (a + cnt + 2) u (window mean of the bin means of |x|)."""
    return (a + 1) * U32 * xabs, (a + cnt[None, :, None] + 2) * U32 * aabs


def pool_is_exact(case, pool_q):
    cnt = (pool_q >= 0).sum(axis=1)
    return case.kind == "exact" and case.a & (case.a - 1) == 0 and bool(np.all(cnt & (cnt - 1) == 0))


# ---- roughness -------------------------------------------------------------------------------------------------------
RoughCase = namedtuple("RoughCase", "b1 b2 T r")
ROUGH_BLOCKS = [(20, 14), (1, 9), (9, 1), (2, 2), (7, 9), (65, 3), (32, 32)]
ROUGH_FRAMES = [3, 4, 255, 256, 257, 513, 777]
ROUGH_ROWS = [1, 9, 64]
ROUGH_CASES = [RoughCase(20, 14, 777, 9), RoughCase(1, 9, 3, 1), RoughCase(9, 1, 4, 9), RoughCase(2, 2, 255, 64),
               RoughCase(7, 9, 256, 9), RoughCase(65, 3, 257, 64), RoughCase(32, 32, 513, 9), RoughCase(20, 14, 3, 64),
               RoughCase(32, 32, 777, 1), RoughCase(7, 9, 4, 1)]
ROUGH_TILES = 6
ROUGH_KINDS = ("smooth", "white", "single", "zero")
ROUGH_SHARP = 1e-5
ROUGH_MUTATIONS_T = ("ends", "t_minus_1")
ROUGH_MUTATIONS_S = ("across_columns", "count_b1b2")


def rough_kind(tile, c):
    return ROUGH_KINDS[(tile + c) % 4]


def rough_inputs(case):
    """U float32 (tiles, r, d) with pixel q = i + b1 j, V float32 (tiles, r, T); row (tile, c) is of rough_kind(tile, c).
    A smooth trace has a period of 16 frames: its second difference is 0.15 of its size, so the cancellation in
    v[t-1] + v[t+1] - 2 v[t] costs a factor ~13 in relative error, not more."""
    rng = np.random.default_rng(case.b1 * 100000 + case.b2 * 1000 + case.T)
    b1, b2, T, r = case
    d = b1 * b2
    U = np.zeros((ROUGH_TILES, r, d), dtype=np.float32)
    V = np.zeros((ROUGH_TILES, r, T), dtype=np.float32)
    ii, jj = np.meshgrid(np.arange(b1), np.arange(b2), indexing="ij")
    tt = np.arange(T)
    for t in range(ROUGH_TILES):
        for c in range(r):
            kind = rough_kind(t, c)
            if kind == "smooth":
                img = 2.0 + np.cos(0.3 * ii + rng.uniform(0, 6)) * np.cos(0.2 * jj + rng.uniform(0, 6))
                U[t, c] = (rng.uniform(0.5, 20) * img).flatten(order="F")
                phase = rng.uniform(0, 6) if T >= 16 else np.pi / 2 - np.pi * (T - 1) / 16    # a short trace: its crest
                V[t, c] = rng.uniform(0.5, 20) * (np.sin(2 * np.pi * tt / 16 + phase) + 0.01 * rng.standard_normal(T))
            elif kind == "white":
                U[t, c] = rng.standard_normal(d) * rng.uniform(0.5, 20)
                V[t, c] = rng.standard_normal(T) * rng.uniform(0.5, 20)
            elif kind == "single":
                U[t, c, rng.integers(d)] = 3.5
                V[t, c, rng.integers(T)] = -2.5
    return U, V


def spatial_stat(u, b1, b2, mutation=None):
    """evaluation.py:84-111 in float64 on one component, with a running bound of the kernel's fp32 error.  Returns
    (stat, bound): stat is NaN for the zero image (0 / 0) and the bound is then NaN too.
    Error model of spatial_stat_kernel: every |difference| is one rounded subtraction (u relative); a lane adds
    ceil(d / 64) terms, six butterfly steps follow, all terms non-negative, so each sum is within gamma(chain + 6) of its
    exact value; then the add of the two difference sums, the division by the count, the division by d and the quotient."""
    img = np.asarray(u, dtype=np.float64).reshape((b1, b2), order="F")
    d = b1 * b2
    vert = np.abs(img[1:, :] - img[:-1, :]).sum()
    if mutation == "across_columns":          # q + 1 taken as the vertical neighbour whatever the column
        flat = img.flatten(order="F")
        vert = np.abs(flat[1:] - flat[:-1]).sum()
    horiz = np.abs(img[:, :-1] - img[:, 1:]).sum()
    count = (b1 - 1) * b2 + b1 * (b2 - 1)
    if mutation == "count_b1b2":
        count = (b1 - 1) * b2 + b1 * b2
    with np.errstate(divide="ignore", invalid="ignore"):
        stat = np.float64(vert + horiz) / count / (np.abs(img).sum() / d)
    k = -(-d // 64) + 6
    num_rel = (1 + U32) * (1 + gamma(k, U32)) * (1 + U32) - 1      # subtraction, sums, sv + sh
    den_rel = gamma(k, U32)
    rel = (1 + num_rel) * (1 + U32) ** 2 / ((1 - den_rel) * (1 - U32)) - 1
    return stat, abs(stat) * rel


def temporal_stat(v, mutation=None):
    """evaluation.py:114-126 in float64 on one trace, with a running bound of the kernel's fp32 error.
    Error model of temporal_stat_kernel: s = fl(v[t-1] + v[t+1]) errs by u |v[t-1] + v[t+1]|, fl(s - 2 v[t]) adds u times
    its result (2 v[t] is exact, fused or not): the numerator's terms carry an ABSOLUTE error u (|v[t-1] + v[t+1]| (1 + u) +
    |second difference|) each.  A lane adds ceil(T / 256) terms, six butterfly steps and three cross-wave adds follow:
    gamma(chain + 9) on either sum; then the two divisions by the counts and the quotient."""
    v = np.asarray(v, dtype=np.float64)
    T = v.size
    pair = v[:-2] + v[2:]
    d2 = np.abs(pair - 2.0 * v[1:-1])
    num = d2.sum()
    term_err = U32 * ((1 + U32) * np.abs(pair) + d2).sum()
    if mutation == "ends":                    # t = 0 and t = T - 1 in the numerator, the missing neighbour as zero
        num = num + abs(v[1] - 2.0 * v[0]) + abs(v[-2] - 2.0 * v[-1])
    n_mean = T - 1 if mutation == "t_minus_1" else T - 2
    den = np.abs(v).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        stat = np.float64(num) / n_mean / (den / T)
        k = -(-T // 256) + 9
        num_rel = (1 + np.float64(term_err) / num) * (1 + gamma(k, U32)) - 1
        den_rel = gamma(k, U32)
        rel = (1 + num_rel) * (1 + U32) ** 2 / ((1 - den_rel) * (1 - U32)) - 1
    return stat, abs(stat) * rel


def rough_reference(case, U, V):
    """(stats, bounds), each (tiles, r, 2) float64"""
    stats = np.zeros(U.shape[:2] + (2,))
    bounds = np.zeros_like(stats)
    for t in range(U.shape[0]):
        for c in range(U.shape[1]):
            stats[t, c, 0], bounds[t, c, 0] = spatial_stat(U[t, c], case.b1, case.b2)
            stats[t, c, 1], bounds[t, c, 1] = temporal_stat(V[t, c])
    return stats, bounds


def rough_u_ld(d):
    return tile_gemm_ref.tile_dpad(d) + 4


def rough_v_ld(T):
    return tile_gemm_ref.time_ld(T)
