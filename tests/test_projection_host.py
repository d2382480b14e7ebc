"""Host side of the projection onto a stored basis (localmd_amd/projection.py): group tables, their validation, the
identity the GPU tests rely on, and argument checks.  No device needed."""
import os

import numpy as np
import pytest
import scipy.sparse

from localmd_amd import projection as P
from localmd_amd.pmdarray import PMDArray
from localmd_amd.synthetic import make_movie

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_small.npz")


def _fixture_u():
    d = np.load(GOLDEN)
    u = scipy.sparse.csr_matrix((d["U_data"], d["U_indices"], d["U_indptr"]), shape=tuple(d["U_shape"]))
    return u, d


def _random_tiled_u(d1, d2, b1, b2, order, K, seed):
    """A decomposition-shaped U: tiles on two grids shifted by half a tile, 0..7 columns each with exact zeros dropped
    (as dia.dot(coo) does), then K dense background columns (K = 0: one empty placeholder column)."""
    rng = np.random.default_rng(seed)
    D = d1 * d2
    ids = np.arange(D).reshape((d1, d2), order=order)
    cols = []
    for s1, s2 in ((0, 0), (b1 // 2, b2 // 2)):
        for i0 in range(s1, d1 - b1 + 1, b1):
            for j0 in range(s2, d2 - b2 + 1, b2):
                rows = ids[i0:i0 + b1, j0:j0 + b2].reshape(-1)
                for _ in range(int(rng.integers(0, 8))):
                    v = rng.standard_normal(rows.size)
                    v[rng.random(rows.size) < 0.1] = 0.0
                    cols.append((rows, v))
    for _ in range(max(K, 0)):
        cols.append((np.arange(D), rng.standard_normal(D)))
    if K <= 0:
        cols.append((np.zeros(0, np.int64), np.zeros(0)))
    r = np.concatenate([c[0] for c in cols])
    c = np.concatenate([np.full(len(x[0]), k) for k, x in enumerate(cols)])
    v = np.concatenate([x[1] for x in cols])
    keep = v != 0
    return scipy.sparse.coo_matrix((v[keep], (r[keep], c[keep])), shape=(D, len(cols))).tocsr()


def _scatter_back(t, fov, order):
    """U (in its own row order) rebuilt from the group tables alone; also checks the per-group limits."""
    d1, d2 = fov
    D = d1 * d2
    u_of_c = np.arange(D).reshape((d1, d2), order=order).reshape(-1)   # C-order id -> U row
    out = np.zeros((D, t["n_cols"]), dtype=np.float32)
    hits = np.zeros((D, t["n_cols"]), dtype=np.int64)
    for (pix_off, p, a_off, out_row, r, to_ws), col0 in zip(t["groups"], t["col0"]):
        assert 1 <= r <= P.MAX_ROWS and 0 <= p <= P.P_MAX
        rp, pp = P._pad(r, P.ROW_PAD), P._pad(p, P.PIX_PAD)
        blk = t["a"][a_off:a_off + rp * pp].reshape(rp, pp)
        assert not blk[r:].any() and not blk[:, p:].any()      # padding is zero
        pix = t["pix"][pix_off:pix_off + p]
        assert np.all(np.diff(pix) > 0)
        rows = u_of_c[pix]
        out[rows[:, None], col0 + np.arange(r)[None, :]] += blk[:r, :p].T
        hits[rows[:, None], col0 + np.arange(r)[None, :]] += 1
    assert hits.max() <= 1          # no (pixel, column) entry is written twice
    return out


def _check_cover(t):
    """Every column lands in exactly one direct group, or in every chunk of one wide set (rows of the wide table)."""
    n = t["n_cols"]
    direct = np.zeros(n, np.int64)
    for (pix_off, p, a_off, out_row, r, to_ws), col0 in zip(t["groups"], t["col0"]):
        if to_ws == 0:
            assert out_row == col0
            direct[col0:col0 + r] += 1
    wide = np.zeros(n, np.int64)
    for z_row, row0, parts, stride in t["wide"]:
        wide[z_row] += 1
        chunk_rows = row0 + stride * np.arange(parts)
        owners = [g for g in t["groups"] if g[5] == 1 and g[3] <= chunk_rows[0] < g[3] + g[4]]
        assert len(owners) == 1
    assert np.all(direct + wide == 1), (direct, wide)


def test_group_tables_rebuild_oracle_fixture():
    u, d = _fixture_u()
    fov = tuple(int(x) for x in d["mean_img"].shape)
    t = P.group_tables(u, fov, "F")
    assert np.array_equal(_scatter_back(t, fov, "F"), u.toarray().astype(np.float32))
    _check_cover(t)


@pytest.mark.parametrize("order", ["C", "F"])
def test_group_tables_rebuild_random_tiles(order):
    fov = (40, 48)
    u = _random_tiled_u(*fov, 10, 12, order, K=0, seed=5 if order == "C" else 6)
    t = P.group_tables(u, fov, order)
    assert np.array_equal(_scatter_back(t, fov, order), u.toarray().astype(np.float32))
    _check_cover(t)
    assert len(t["wide"]) == 0 and t["n_partial_rows"] == 0
    # one group per tile: no group spans two tile rectangles (every tile here has 120 pixels)
    assert t["groups"][:, 1].max() <= 120


@pytest.mark.parametrize("order", ["C", "F"])
def test_group_tables_split_background_columns(order):
    fov = (60, 70)          # 4200 pixels: a dense column is three P_MAX chunks
    K = 3
    u = _random_tiled_u(*fov, 20, 14, order, K=K, seed=7)
    t = P.group_tables(u, fov, order)
    assert np.array_equal(_scatter_back(t, fov, order), u.toarray().astype(np.float32))
    _check_cover(t)
    assert len(t["wide"]) == K
    parts = -(-fov[0] * fov[1] // P.P_MAX)
    assert np.all(t["wide"][:, 2] == parts) and t["n_partial_rows"] == parts * K
    assert np.array_equal(t["wide"][:, 0], np.arange(u.shape[1] - K, u.shape[1]))


def test_group_tables_pixel_ids_are_c_order():
    """A single column on pixel (i, j) gets the id i * d2 + j whatever the decomposition's order."""
    d1, d2 = 5, 7
    for order in ("C", "F"):
        urow = np.arange(d1 * d2).reshape((d1, d2), order=order)[2, 3]
        u = scipy.sparse.csr_matrix((np.array([1.5]), (np.array([urow]), np.array([0]))), shape=(d1 * d2, 1))
        t = P.group_tables(u, (d1, d2), order)
        assert t["pix"].tolist() == [2 * d2 + 3]


def test_empty_column_gets_a_zero_row():
    u = _random_tiled_u(20, 24, 10, 12, "F", K=0, seed=3)
    t = P.group_tables(u, (20, 24), "F")
    last = u.shape[1] - 1
    g = [g for g, c0 in zip(t["groups"], t["col0"]) if c0 <= last < c0 + g[4]]
    assert len(g) == 1 and g[0][5] == 0


def test_validate_tables_rejects_faults():
    u, d = _fixture_u()
    t = P.group_tables(u, d["mean_img"].shape, "F")
    for key, edit in [
        ("pix", lambda x: x.__setitem__(0, t["D"])),
        ("pix", lambda x: x.__setitem__(0, -1)),
        ("groups", lambda x: x.__setitem__((1, 0), x[1, 0] + 1)),        # offsets no longer consecutive
        ("groups", lambda x: x.__setitem__((0, 4), 65)),                 # more than 64 rows
        ("groups", lambda x: x.__setitem__((0, 2), x[0, 2] + 16)),       # A offsets
        ("groups", lambda x: x.__setitem__((0, 3), t["n_cols"])),        # output rows outside Z
    ]:
        bad = dict(t)
        bad[key] = t[key].copy()
        edit(bad[key])
        with pytest.raises(ValueError):
            P.validate_tables(bad)


def test_fixture_identity_fp64():
    """(U R)^T Y_std = diag(s) Vt on the oracle fixture, its movie regenerated by make_movie, in fp64 NumPy.
    Measured: 1.01e-6 normwise (the fixture's float32 R / s / Vt); bound 3e-6."""
    u, d = _fixture_u()
    T, d1, d2 = (int(x) for x in d["movie_shape"])
    Y = make_movie(T, d1, d2, seed=int(d["movie_seed"])).astype(np.float64)
    Ys = (Y - d["mean_img"]) / d["std_img"]
    Yu = np.stack([f.reshape(-1, order="F") for f in Ys])        # pixels in U's (F) row order
    C = (u @ d["R"].astype(np.float64)).T @ Yu.T
    ref = d["s"].astype(np.float64)[:, None] * d["Vt"]
    err = np.linalg.norm(C - ref) / np.linalg.norm(ref)
    assert err < 3e-6, err


def test_fov_mismatch_raises_before_any_context(monkeypatch):
    from localmd_amd import _lib

    def no_context(*a, **k):
        raise AssertionError("a Context was created")

    monkeypatch.setattr(_lib.Context, "__init__", no_context)
    u, d = _fixture_u()
    pmd = PMDArray(u, d["R"], d["s"], d["Vt"], (400, 30, 36), "F", d["mean_img"], d["std_img"])
    with pytest.raises(ValueError):
        pmd.project_frames(np.zeros((3, 30, 35), np.float32))
    with pytest.raises(ValueError):
        pmd.project_frames(np.zeros((36, 30), np.float32))
    import localmd_amd

    with pytest.raises(ValueError):
        localmd_amd.project_movie(pmd, np.zeros((3, 31, 36), np.uint16))


def test_zero_frames_need_no_device(monkeypatch):
    from localmd_amd import _lib

    monkeypatch.setattr(_lib.Context, "__init__", lambda *a, **k: (_ for _ in ()).throw(AssertionError("Context")))
    u, d = _fixture_u()
    pmd = PMDArray(u, d["R"], d["s"], d["Vt"], (400, 30, 36), "F", d["mean_img"], d["std_img"])
    c = pmd.project_frames(np.zeros((0, 30, 36), np.float32))
    assert c.shape == (39, 0) and c.dtype == np.float32
