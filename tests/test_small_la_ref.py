"""Host checks of tests/small_la_ref.py: the generators produce the ranks, condition numbers and spectral gaps the GPU tests
of tests/test_gpu_tile_small_la.py rely on, the restated QR kernel is the factorisation it claims to be and stays inside
the outer caps with fp32 storage, and the bounds of the pooling and roughness tests are sharp (below 1e-5 relative) and
effective (every mutated reference lands outside them)."""
import numpy as np
import pytest

from oracle import pmd_oracle as O
from tests import small_la_ref as R


# ---- small_qr --------------------------------------------------------------------------------------------------------
def test_qr_storage_rule_and_limits():
    """pmd_launch_small_qr re-derived: at l = 60 the fp64 copy needs 60 ldm 8 + 2608 <= 150 KB, ldm = P | 1 <= 314.6, odd:
    P <= 313; at l = 64 the fp32 copy needs 64 ldm 4 + 2608 <= 160 KB, ldm <= 629.8: P <= 629."""
    assert R.QR_TAIL_BYTES == 2608
    want = {(313, 60): "f64", (314, 60): "f32", (629, 64): "f32", (628, 64): "f32", (630, 64): None, (10, 65): None}
    for shape, storage in want.items():
        assert R.qr_storage(*shape) == storage, shape
    assert max(P for P in range(1, 700) if R.qr_storage(P, 60) == "f64") == 313
    assert max(P for P in range(1, 700) if R.qr_storage(P, 64) is not None) == 629
    assert set(want) <= set(R.QR_SHAPES) | set(R.QR_UNSUPPORTED)
    assert all(R.qr_storage(P, l) == "f64" for P, l in R.QR_SHAPES if P <= 313)
    assert sorted(s for s in R.QR_SHAPES if R.qr_storage(*s) == "f32") == [(314, 60), (628, 64), (629, 64)]
    assert {P % 2 for P, l in R.QR_SHAPES if l == 60} == {0, 1}          # ldm = P | 1: P + 1 and P


@pytest.mark.parametrize("P,l", R.QR_SHAPES)
def test_qr_tiles_are_what_their_names_say(P, l):
    tiles = R.qr_tiles(P, l)
    nref = min(P, l)
    assert len(tiles) == len(R.QR_TILE_KINDS) and all(Y.shape == (P, l) and Y.dtype == np.float32 for Y in tiles)
    rank = lambda Y: int(np.linalg.matrix_rank(Y.astype(np.float64), tol=1e-5 * np.linalg.norm(Y.astype(np.float64), 2)))
    for b, kind in enumerate(R.QR_TILE_KINDS):
        Y = tiles[b]
        if kind == "well":
            assert b in R.QR_WELL and R.qr_cond(Y) <= R.QR_COND_MAX, (b, R.qr_cond(Y))
            assert rank(Y) == nref
        elif kind == "graded":
            norms = np.linalg.norm(Y.astype(np.float64), axis=0)
            assert l < 3 or norms.max() / norms.min() > 100
            assert rank(Y / np.maximum(norms, 1e-30)[None, :]) == nref
        elif kind == "rank5":
            assert rank(Y) == min(5, nref)
        elif kind == "zero_tail":
            assert np.all(Y[:, l - l // 2:] == 0) and rank(Y) == min(P, l - l // 2)
        else:
            assert np.all(Y == Y[:1]) and rank(Y) == 1
    assert not np.array_equal(tiles[0], tiles[1])


@pytest.mark.parametrize("P,l", [s for s in R.QR_SHAPES if R.qr_storage(*s) == "f64"])
def test_qr_restatement_in_fp64_storage(P, l):
    """With fp64 storage the restatement is Householder QR in float64 plus the output rounding: it meets the distance
    bound on the well-conditioned tiles and the derived orthonormality and projection bounds on every tile."""
    for b, Y in enumerate(R.qr_tiles(P, l)):
        Q = R.qr_restated(Y, "f64")
        Q64 = R.qr_reference(Y) if b in R.QR_WELL else None
        orth, proj, _ = R.qr_figures(Q, Y)
        assert orth <= R.qr_orth_bound(P), (b, orth)
        assert proj <= R.qr_proj_bound(Y), (b, proj, R.qr_proj_bound(Y))
        if Q64 is not None:
            err = np.abs(Q.astype(np.float64) - Q64)
            assert np.all(err <= R.qr_dist_bound(Q64, R.qr_cond(Y), P)), (b, float(err.max()))


@pytest.mark.parametrize("P,l", [s for s in R.QR_SHAPES if R.qr_storage(*s) == "f32"])
def test_qr_restatement_in_fp32_storage_stays_inside_the_caps(P, l):
    """The figures the GPU is held to FACTOR times of: orthonormality below 5e-6, projection below 1e-4 max(max|Y|, 1),
    and on the well-conditioned tiles a distance to Q64 that is that of fp32 storage (above the fp64 bound, below 1e-4)."""
    for b, Y in enumerate(R.qr_tiles(P, l)):
        Q = R.qr_restated(Y, "f32")
        orth, proj, dist = R.qr_figures(Q, Y, R.qr_reference(Y) if b in R.QR_WELL else None)
        assert 0 < R.FACTOR * orth <= R.QR_ORTH_CAP, (b, orth)
        assert 0 < R.FACTOR * proj <= R.qr_proj_cap(Y), (b, proj)
        if dist is not None:
            assert 1e-8 < dist < 1e-4, (b, dist)


@pytest.mark.parametrize("P,l", [(25, 20), (7, 20), (314, 60)])
def test_qr_restatement_is_scale_covariant(P, l):
    """Every operation of the algorithm is exact under a power-of-two scale and the dependence test is relative: the
    restatement gives the same bits for Y 2^24 and Y 2^-24, the constant and the rank-5 tile included."""
    storage = R.qr_storage(P, l)
    for Y in R.qr_tiles(P, l):
        Q = R.qr_restated(Y, storage)
        for s in R.SCALES:
            assert np.array_equal(R.qr_restated(Y * np.float32(s), storage).view(np.int32), Q.view(np.int32)), s


def test_qr_dependence_rule_cuts_the_constant_tile():
    """Identical rows: after the first reflector only rounding residue is left below the diagonal, and the rule gives the
    remaining columns tau = 0 - Q is then the first reflector applied to unit vectors, orthonormal to rounding."""
    Y = R.qr_tiles(25, 20)[5]
    for storage in ("f64", "f32"):
        Q = R.qr_restated(Y, storage).astype(np.float64)
        assert np.abs(np.abs(Q[:, 0]) - 0.2).max() < 1e-7          # 1 / sqrt(25) in every row
        assert np.abs(Q.T @ Q - np.eye(20)).max() < 4e-7


# ---- small_eig -------------------------------------------------------------------------------------------------------
# (kind, order) whose reference spectrum has an eigenvalue within a factor 100 of 1e-10 lambda_max: the rows over four
# decades of the project's own family put their smallest eigenvalue at 0.6 .. 0.95e-8 lambda_max, and the fp32 product of
# gram_lowrank leaves rounding eigenvalues of 5e-12 .. 9e-9 lambda_max on both sides of the threshold.  The GPU test
# compares with the reference's classification eigenvalue by eigenvalue where it is pinned (eig_expected_keep: further
# from the threshold than twice the eigenvalue bound of mode 0, which is asserted on the same input, so no solver that
# passes mode 0 can classify it the other way).  That is every eigenvalue of every matrix here but at most one rounding
# eigenvalue of a gram_lowrank matrix; and in every case the zero pattern must be the rule applied to the eigenvalues the
# call itself returned.
EIG_UNDECIDED = ({("gram_lowrank", n) for n in (5, 31, 32, 33, 50, 63, 64)} |
                 {("decades", n) for n in (2, 3, 4, 5, 32, 33, 50, 63, 64)})


def test_eig_inputs():
    seen = set()
    for n in R.EIG_ORDERS:
        mats = R.eig_mats(n)
        assert len(mats) == len(R.EIG_KINDS) == 16
        for kind, M in zip(R.EIG_KINDS, mats):
            assert M.shape == (n, n) and M.dtype == np.float64 and np.isfinite(M).all()
            w = np.linalg.eigvalsh(M)
            if not R.eig_decided(w):
                seen.add((kind, n))
            top = np.abs(w).max()
            keep, pinned = R.eig_expected_keep(w[::-1], 1e-10)
            # (the zero matrix: exact zeros, zeroed by lambda <= 0)
            assert pinned.all() or not M.any() or kind == "gram_lowrank", (kind, n)
            assert pinned.sum() >= n - 1 or not M.any()
            keep0, pinned0 = R.eig_expected_keep(w[::-1], 0.0)
            assert np.all(pinned0 | (np.abs(w[::-1]) <= 1e-11 * top)) and np.all(keep0[pinned0] == (w[::-1][pinned0] > 0))
            if kind == "nulls":
                assert int((np.abs(w) < 1e-12 * top).sum()) == R.eig_nnull(n)
            if kind == "indefinite" and n >= 2:
                assert w[0] < -0.9 and w[-1] > 0.9
            if kind == "repeated" and n >= 8:
                assert np.abs(w[:n // 4] - 1.0).max() < 1e-5
            if kind == "zero":
                assert not M.any()
            if kind in ("diagonal", "tridiagonal"):
                assert not np.triu(M, 2).any()         # the sigma == 0 shortcut of the tridiagonalisation
    assert seen == EIG_UNDECIDED, sorted(seen ^ EIG_UNDECIDED)


@pytest.mark.parametrize("slices", R.EIG_SLICES)
def test_eig_slices_need_the_sum_and_the_symmetrisation(slices):
    for n in (1, 5, 33):
        mats = R.eig_mats(n)
        G = R.eig_slices(mats, slices, np.nan, seed=n)
        assert G.shape == (16, slices, 64, 64)
        assert np.isnan(G[:, :, n:, :]).all() and np.isnan(G[:, :, :, n:]).all() and np.isfinite(G[:, :, :n, :n]).all()
        M = R.eig_matrix_of(G, n)
        assert np.array_equal(M, np.swapaxes(M, 1, 2))
        for b, kind in enumerate(R.EIG_KINDS):
            top = np.abs(mats[b]).max()
            assert np.abs(M[b] - mats[b]).max() <= 1e-14 * top, (kind, n)
            if n > 1 and top > 0:
                for k in range(slices):
                    blk = G[b, k, :n, :n]
                    assert np.abs(blk - blk.T).max() > 0, (kind, "a symmetric slice")
                    assert slices == 1 or np.abs(blk - mats[b]).max() > 0.1 * np.abs(mats[b]).max(), (kind, "a full share")
            if kind in ("diagonal", "tridiagonal", "zero", "identity"):
                assert np.array_equal(M[b], mats[b]), (kind, "exact zeros must survive the split")
        for s in R.EIG_SCALES:
            assert np.array_equal(R.eig_matrix_of(G * s, n), M * s)
        Z = R.eig_slices(mats, slices, 0.0, seed=n)
        assert np.array_equal(Z[:, :, :n, :n], G[:, :, :n, :n]) and not Z[:, :, n:, :].any()


def test_eig_keep_rule():
    lam = np.array([[4.0, 1.0, 1e-11, 0.0, -1e-30, -3.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    assert R.eig_keep_rule(lam, 0.0).tolist() == [[True, True, True, False, False, False], [False] * 6]
    assert R.eig_keep_rule(lam, 1e-10).tolist() == [[True, True, False, False, False, False], [False] * 6]


# ---- tile_pool_bin ---------------------------------------------------------------------------------------------------
def _pool_fp32_chains(X, pix, pool_q, a, nbins):
    """bin_average_kernel and tile_pool_kernel operation by operation in float32"""
    f = np.float32
    s = np.zeros((X.shape[0], nbins), dtype=f)
    for tau in range(a):
        s = s + X[:, tau:a * nbins:a][:, :nbins]
    xbar = s * (f(1) / f(a))
    abar = np.zeros((pix.shape[0], pool_q.shape[0], nbins), dtype=f)
    for p in range(pool_q.shape[0]):
        acc = np.zeros((pix.shape[0], nbins), dtype=f)
        for q in pool_q[p]:
            if q >= 0:
                acc = acc + xbar[pix[:, q]]
        abar[:, p] = acc * (f(1) / f((pool_q[p] >= 0).sum()))
    return xbar, abar


def test_pool_cases_cover_the_issue():
    by = {c.name: c for c in R.POOL_CASES}
    assert len(by) == len(R.POOL_CASES)
    made = {name: R.pool_inputs(c) for name, c in by.items() if name != "tiles_two_chunks"}
    counts = lambda name: sorted(set((made[name]["pool_q"] >= 0).sum(axis=1).tolist()))
    assert counts("v0") == [4] and counts("partial2") == [1, 2, 4] and counts("partial3") == [4, 6, 9]
    assert (made["partial2"]["pool_q"] < 0).any() and made["pool1"]["pool_q"].shape == (35, 1)
    assert {c.a for c in R.POOL_CASES} >= {1, 4, 10}
    assert by["partial2"].T % by["partial2"].a and by["a4_random_pix"].T % 4
    assert made["bins2100"]["nbins"] == 2100 > 8 * 256 and by["bins2100"].a == 1
    rows = made["rows_two_chunks"]
    assert rows["X"].shape[0] == 32768 + 70 and rows["pix"].max() >= 32768 > rows["pix"].min()
    assert by["tiles_two_chunks"].n_tiles == 32768 + 3 and by["tiles_two_chunks"].block == (2, 2)
    assert any(c.extra > 0 for c in R.POOL_CASES)
    assert R.pool_is_exact(by["exact"], made["exact"]["pool_q"]) and not R.pool_is_exact(by["v0"], made["v0"]["pool_q"])


@pytest.mark.parametrize("case", [c for c in R.POOL_CASES if c.name != "tiles_two_chunks"], ids=lambda c: c.name)
def test_pool_bounds_are_sharp_and_effective(case):
    inp = R.pool_inputs(case)
    X, pix, pool_q, nbins, a = inp["X"], inp["pix"], inp["pool_q"], inp["nbins"], case.a
    xbar, xabs, abar, aabs, cnt = R.pool_reference(X, pix, pool_q, a, nbins)
    bx, ba = R.pool_bounds(a, xabs, aabs, cnt)
    assert (a + cnt.max() + 2) * R.U32 < 1e-5                     # sharp: relative to the mean of |x|
    fx, fa = _pool_fp32_chains(X, pix, pool_q, a, nbins)
    assert np.all(np.abs(fx - xbar) <= bx) and np.all(np.abs(fa - abar) <= ba)   # the fp32 chains themselves pass
    if R.pool_is_exact(case, pool_q):
        assert np.array_equal(fx.astype(np.float64), xbar) and np.array_equal(fa.astype(np.float64), abar)
        return
    # the oracle's pooling where the blocks are the grid's and divide evenly
    if case.fov is not None and all(b % case.pool == 0 for b in case.block):
        d1, d2 = case.fov
        mov = X[:, :a * nbins].astype(np.float64).reshape(d1, d2, a * nbins)
        for t, (k, j) in enumerate(inp["origins"]):
            ds = O.downsample_average_pooling(mov[k:k + case.block[0], j:j + case.block[1]], case.pool)
            ref = np.mean(np.reshape(ds, (ds.shape[0] * ds.shape[1], a, nbins), order="F"), axis=1)
            assert np.abs(ref - abar[t]).max() <= 1e-12 * np.abs(X).max()
    # mutations: bins shifted by one frame; partial windows divided by the full window size
    if case.T > a * nbins or a > 1:
        shifted = np.roll(X, -1, axis=1)
        assert np.mean(np.abs(R.pool_reference(shifted, pix, pool_q, a, nbins)[2] - abar) > ba) > 0.99
    if (pool_q < 0).any():
        wrong = abar * (cnt / pool_q.shape[1])[None, :, None]
        partial = cnt < pool_q.shape[1]
        assert np.mean(np.abs(wrong - abar)[:, partial] > ba[:, partial]) > 0.99


# ---- roughness -------------------------------------------------------------------------------------------------------
def test_rough_cases_cover_the_issue():
    assert {(c.b1, c.b2) for c in R.ROUGH_CASES} == set(R.ROUGH_BLOCKS)
    assert {c.T for c in R.ROUGH_CASES} == set(R.ROUGH_FRAMES)
    assert {c.r for c in R.ROUGH_CASES} == set(R.ROUGH_ROWS)
    for c in R.ROUGH_CASES:
        assert {R.rough_kind(t, k) for t in range(R.ROUGH_TILES) for k in range(c.r)} == set(R.ROUGH_KINDS)


@pytest.mark.parametrize("case", R.ROUGH_CASES, ids=lambda c: "%dx%d_T%d_r%d" % c)
def test_rough_bounds_are_sharp_and_effective(case):
    U, V = R.rough_inputs(case)
    stats, bounds = R.rough_reference(case, U, V)
    for t in range(R.ROUGH_TILES):
        for c in range(case.r):
            kind = R.rough_kind(t, c)
            if kind == "zero":
                assert np.isnan(stats[t, c]).all()           # 0 / 0, as in the reference
                continue
            assert np.all(np.isfinite(stats[t, c])) and np.all(stats[t, c] >= 0)
            assert np.all(bounds[t, c] < R.ROUGH_SHARP * stats[t, c]), (t, c, kind, bounds[t, c] / stats[t, c])
            img = U[t, c].astype(np.float64).reshape((case.b1, case.b2), order="F")
            assert abs(O.spatial_roughness_stat(img) - stats[t, c, 0]) <= 1e-12 * stats[t, c, 0]
            assert abs(O.temporal_roughness_stat(V[t, c].astype(np.float64)) - stats[t, c, 1]) <= 1e-12 * stats[t, c, 1]
            if kind == "single":
                continue                                     # a mutation may leave a single pixel or frame alone
            for m in R.ROUGH_MUTATIONS_S:
                mutated = R.spatial_stat(U[t, c], case.b1, case.b2, m)[0]
                if m == "across_columns" and case.b2 == 1:
                    assert mutated == stats[t, c, 0]         # one column: there is no boundary to cross
                else:
                    assert abs(mutated - stats[t, c, 0]) > bounds[t, c, 0], (t, c, kind, m)
            for m in R.ROUGH_MUTATIONS_T:
                assert abs(R.temporal_stat(V[t, c], m)[0] - stats[t, c, 1]) > bounds[t, c, 1], (t, c, kind, m)


def test_rough_smooth_rows_are_smoother_than_white_ones():
    case = R.RoughCase(20, 14, 777, 9)
    stats, _ = R.rough_reference(case, *R.rough_inputs(case))
    kinds = np.array([[R.rough_kind(t, c) for c in range(case.r)] for t in range(R.ROUGH_TILES)])
    assert stats[kinds == "smooth"].max() < 0.5 < 1.0 < stats[kinds == "white"].min()
