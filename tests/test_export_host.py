"""Host side of the streamed export (localmd_amd.export_movie, localmd_amd/export.py): argument checks before any device
work or file, the block plan and the memory estimate, the per-patch tables of pmd_group_expand (checked by a NumPy
emulation of the kernel's sum), the streaming TIFF writer and the NumPy quantiser.  No device needed: without one,
Context(0) raises, so a ValueError here shows the check ran first."""
import os

import numpy as np
import pytest
import scipy.sparse

import localmd_amd
from localmd_amd import _lib
from localmd_amd import export as E
from localmd_amd import projection as P
from localmd_amd._minitiff import TiffWriter, tiff_needs_bigtiff, write_tiff
from localmd_amd.dataset import TiffArray
from localmd_amd.pmdarray import PMDArray

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_small.npz")


def _pmd(T=300, d1=6, d2=7, rank=3, order="F"):
    rng = np.random.default_rng(0)
    D = d1 * d2
    u = scipy.sparse.random(D, 4, density=0.5, random_state=1, format="coo")
    return PMDArray(u, rng.standard_normal((4, rank)), np.ones(rank), rng.standard_normal((rank, T)), (T, d1, d2), order,
                    rng.standard_normal((d1, d2)), np.ones((d1, d2)))


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a device context fails the test: the checks must come first."""
    def refuse(*a, **k):
        raise AssertionError("a device context was opened before the argument checks")
    monkeypatch.setattr(_lib.Context, "__init__", refuse)


def test_reexported():
    assert localmd_amd.export_movie is E.export_movie
    assert callable(PMDArray.export)


# ---- argument errors -----------------------------------------------------------------------------------------------
def _bad_calls(tmp_path):
    pmd = _pmd()
    mov = np.zeros((300, 6, 7), np.float32)
    tif = str(tmp_path / "o.tif")
    return pmd, [
        (ValueError, dict(out=tif, panels="noise")),
        (ValueError, dict(out=tif, panels=("raw", "raw"), movie=mov)),
        (ValueError, dict(out=tif, panels=())),
        (ValueError, dict(out=tif, panels=("raw", "denoised"))),                # raw without a movie
        (ValueError, dict(out=tif, panels="residual")),                         # residual without a movie
        (ValueError, dict(out=tif, panels="raw", movie=np.zeros((300, 6, 8), np.float32))),
        (ValueError, dict(out=tif, panels="raw", movie=np.zeros((299, 6, 7), np.float32))),
        (ValueError, dict(out=tif, dtype="float64")),
        (ValueError, dict(out=tif, dtype="uint8")),
        (ValueError, dict(out=str(tmp_path / "o.png"))),
        (ValueError, dict(out=str(tmp_path / "o"))),
        (ValueError, dict(out=np.zeros((300, 6, 7), np.float32), panels=("raw", "denoised"), movie=mov)),   # width
        (ValueError, dict(out=np.zeros((300, 6, 7), np.float64))),                                          # dtype
        (ValueError, dict(out=np.zeros((300, 6, 7), np.float32), dtype="uint16")),
        (ValueError, dict(out=np.zeros((299, 6, 7), np.float32))),
        (ValueError, dict(out=np.zeros((300, 6, 7), np.float32), bigtiff=True)),
        (TypeError, dict(out=[1, 2, 3])),
    ]


def test_argument_errors_before_any_device_work(no_device, tmp_path):
    pmd, calls = _bad_calls(tmp_path)
    for exc, kw in calls:
        kw = dict(kw)
        out = kw.pop("out")
        with pytest.raises(exc):
            localmd_amd.export_movie(pmd, out, **kw)
        with pytest.raises(exc):
            pmd.export(out, **kw)
    assert os.listdir(tmp_path) == []
    with pytest.raises(TypeError):
        localmd_amd.export_movie(np.zeros((300, 6, 7)), str(tmp_path / "o.tif"))


def test_classic_tiff_too_large_raises_before_any_file(no_device, tmp_path):
    T, d1, d2 = 70000, 128, 128          # 4.6 GB of float32 frames
    pmd = PMDArray(scipy.sparse.coo_matrix((d1 * d2, 1)), np.zeros((1, 1)), np.ones(1), np.zeros((1, T)), (T, d1, d2),
                   "F", np.zeros((d1, d2)), np.ones((d1, d2)))
    with pytest.raises(ValueError, match="classic TIFF"):
        localmd_amd.export_movie(pmd, str(tmp_path / "big.tif"), bigtiff=False)
    assert os.listdir(tmp_path) == []


# ---- plan and memory -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 1023, 1024, 1025, 5000, 40000])
def test_block_plan_covers_once_and_ignores_batch_size(T):
    ref = None
    for fbs in (1, 1024, 2000, 3072, 10000, 10 ** 6):
        plan = E.export_plan(T, fbs)
        blocks = [blk for _, _, bl in plan for blk in bl]
        assert blocks[0][0] == 0 and blocks[-1][1] == T
        assert all(a[1] == b[0] for a, b in zip(blocks, blocks[1:]))
        assert all(c0 % E.EXPORT_BLOCK == 0 and 0 < c1 - c0 <= E.EXPORT_BLOCK for c0, c1 in blocks)
        for b0, b1, bl in plan:
            assert bl[0][0] == b0 and bl[-1][1] == b1
        ref = blocks if ref is None else ref
        assert blocks == ref


def test_memory_estimate_does_not_depend_on_length():
    args = dict(D=512 * 512, esize=2, n_panels=3, out_esize=4, n_cols=54604, rank=10000, n_entries=60000, n_a=5 * 10 ** 7,
                n_patches=4096, needs_movie=True, host_source=True, host_dest=True, factors_on_device=False)
    a = E.export_device_bytes(nb=10240, n_batches=4, **args)
    b = E.export_device_bytes(nb=10240, n_batches=400, **args)
    assert a == b
    # the output ring and the two batch buffers are in it
    assert a > E.HOST_SLOTS * 1024 * 512 * 512 * 3 * 4 + 2 * 10240 * 512 * 512 * 2
    dev_dest = E.export_device_bytes(nb=10240, n_batches=4, **dict(args, host_dest=False))
    assert a - dev_dest == E.HOST_SLOTS * 1024 * 512 * 512 * 3 * 4


# ---- per-patch tables ----------------------------------------------------------------------------------------------
def _random_tiled_u(d1, d2, b1, b2, order, K, seed, merged=False, empty_rows=False):
    """Decomposition-shaped U: tiles on two grids shifted by half a tile, 0..7 columns each with exact zeros dropped, then
    K dense background columns.  merged: the last tile of each row of tiles is widened over the edge remainder;
    empty_rows: a band of pixels no column touches."""
    rng = np.random.default_rng(seed)
    D = d1 * d2
    ids = np.arange(D).reshape((d1, d2), order=order)
    cols = []
    for s1, s2 in ((0, 0), (b1 // 2, b2 // 2)):
        for i0 in range(s1, d1 - b1 + 1, b1):
            for j0 in range(s2, d2 - b2 + 1, b2):
                j1 = d2 if merged and j0 + 2 * b2 > d2 else j0 + b2
                rows = ids[i0:i0 + b1, j0:j1].reshape(-1)
                if empty_rows:
                    rows = rows[(rows % 11) != 3]
                for _ in range(int(rng.integers(0, 8))):
                    v = rng.standard_normal(rows.size)
                    v[rng.random(rows.size) < 0.1] = 0.0
                    cols.append((rows, v))
    for _ in range(K):
        rows = np.arange(D)
        if empty_rows:
            rows = rows[(rows % 11) != 3]
        cols.append((rows, rng.standard_normal(rows.size)))
    if not cols:                                   # no tile drew a column and K == 0: a U without columns
        return scipy.sparse.csr_matrix((D, 0))
    r = np.concatenate([c[0] for c in cols])
    c = np.concatenate([np.full(len(x[0]), k) for k, x in enumerate(cols)])
    v = np.concatenate([x[1] for x in cols])
    keep = v != 0
    return scipy.sparse.coo_matrix((v[keep], (r[keep], c[keep])), shape=(D, len(cols))).tocsr()


def _emulate(tabs, xt, Cm):
    """The sum of pmd_group_expand in fp64 NumPy: x[c] = sum over the entries of c's patch of A_g[:, q]^T C[rows]."""
    D = int(tabs["D"])
    out = np.zeros((D, Cm.shape[1]))
    pp, ent, qm, a = xt["patch_ptr"], xt["entries"], xt["qmap"], tabs["a"]
    for k in range(int(xt["n_patches"])):
        cs = k * E.EXPORT_PATCH + np.arange(E.EXPORT_PATCH)
        for e in range(pp[k], pp[k + 1]):
            a_off, p64, r, c_row0 = (int(x) for x in ent[e])
            q = qm[e * E.EXPORT_PATCH:(e + 1) * E.EXPORT_PATCH]
            ok = (q >= 0) & (cs < D)
            blk = a[a_off:a_off + P._pad(r, P.ROW_PAD) * p64].reshape(-1, p64)[:r].astype(np.float64)
            out[cs[ok]] += blk[:, q[ok]].T @ Cm[c_row0:c_row0 + r]
    return out


def _check_tables(u, fov, order, seed=0):
    tabs = P.group_tables(u, fov, order)
    xt = E.expand_tables(tabs)
    E.validate_expand_tables(xt, tabs["a"].size, tabs["n_cols"], tabs["D"])
    D = fov[0] * fov[1]
    Cm = np.random.default_rng(seed).standard_normal((u.shape[1], 5))
    u_of_c = np.arange(D).reshape(fov, order=order).reshape(-1)
    want = u.astype(np.float32).astype(np.float64)[u_of_c] @ Cm
    np.testing.assert_allclose(_emulate(tabs, xt, Cm), want, rtol=1e-12, atol=1e-12)
    # every (patch, group) pair at most once, entries in group order within a patch
    pp = xt["patch_ptr"]
    for k in range(len(pp) - 1):
        a_offs = xt["entries"][pp[k]:pp[k + 1], 0]
        assert np.all(np.diff(a_offs) > 0)
    return tabs, xt


def test_expand_tables_oracle_fixture():
    d = np.load(GOLDEN)
    u = scipy.sparse.csr_matrix((d["U_data"], d["U_indices"], d["U_indptr"]), shape=tuple(d["U_shape"]))
    _check_tables(u, d["mean_img"].shape, "F")


@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("K", [0, 3])
def test_expand_tables_random_tiles(order, K):
    _check_tables(_random_tiled_u(60, 70, 20, 14, order, K, seed=5), (60, 70), order)


@pytest.mark.parametrize("order", ["C", "F"])
def test_expand_tables_merged_tiles_empty_rows(order):
    _check_tables(_random_tiled_u(31, 37, 10, 8, order, 2, seed=9, merged=True, empty_rows=True), (31, 37), order)


def test_expand_tables_only_wide_columns_and_no_columns():
    fov = (45, 50)
    rng = np.random.default_rng(2)
    u = scipy.sparse.csr_matrix(rng.standard_normal((fov[0] * fov[1], 3)))
    _, xt = _check_tables(u, fov, "F")
    assert len(xt["entries"]) > 0
    u0 = scipy.sparse.csr_matrix((fov[0] * fov[1], 0))
    tabs, xt = _check_tables(u0, fov, "C")
    assert len(xt["entries"]) == 0 and not xt["patch_ptr"].any()


def test_validate_expand_tables_rejects_faults():
    u = _random_tiled_u(40, 44, 20, 22, "F", 1, seed=1)
    tabs = P.group_tables(u, (40, 44), "F")
    xt = E.expand_tables(tabs)
    n_a, n_cols, D = tabs["a"].size, tabs["n_cols"], tabs["D"]
    for key, edit in [
        ("entries", lambda x: x.__setitem__((0, 0), n_a)),              # block outside A
        ("entries", lambda x: x.__setitem__((0, 2), 65)),               # too many rows
        ("entries", lambda x: x.__setitem__((0, 2), 0)),
        ("entries", lambda x: x.__setitem__((0, 3), n_cols)),           # rows outside C
        ("entries", lambda x: x.__setitem__((0, 1), 63)),               # row length not a multiple of 64
        ("qmap", lambda x: x.__setitem__(0, 10 ** 6)),                  # pixel index outside the group
        ("qmap", lambda x: x.__setitem__(0, -2)),
        ("patch_ptr", lambda x: x.__setitem__(-1, x[-1] + 1)),          # offsets do not cover the entries
        ("patch_ptr", lambda x: x.__setitem__(1, x[2] + 1)),            # not monotone
    ]:
        bad = dict(xt)
        bad[key] = xt[key].copy()
        edit(bad[key])
        with pytest.raises(ValueError):
            E.validate_expand_tables(bad, n_a, n_cols, D)


# ---- streaming TIFF writer -----------------------------------------------------------------------------------------
def _frames(dtype, T=13, h=9, w=11, seed=0):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((T, h, w)) * 3000
    return v.astype(np.float32) if dtype == "float32" else np.clip(v, np.iinfo(dtype).min, np.iinfo(dtype).max).astype(dtype)


def _stream(path, a, big, pieces):
    with TiffWriter(path, a.shape, a.dtype, bigtiff=big) as tw:
        t = 0
        for k in pieces:
            tw.write(a[t:t + k] if k != "one" else a[t])
            t += 1 if k == "one" else k
        assert t == len(a)


@pytest.mark.parametrize("dtype", ["uint16", "int16", "float32"])
def test_streaming_writer_matches_write_tiff(tmp_path, dtype):
    a = _frames(dtype)
    ref = tmp_path / "ref.tif"
    write_tiff(str(ref), a)
    for big, pieces in [(None, [0, 5, "one", 1, 6]), (False, [13]), (None, ["one"] * 13)]:
        p = tmp_path / "s.tif"
        _stream(str(p), a, big, pieces)
        assert p.read_bytes() == ref.read_bytes()
    # forced BigTIFF: magic 43, and the same pages
    p = tmp_path / "big.tif"
    _stream(str(p), a, True, [2, 0, 11])
    raw = p.read_bytes()
    assert raw[2:4] == b"\x2b\x00"
    np.testing.assert_array_equal(np.asarray(TiffArray(str(p))[0:13]), a.astype(np.float32))
    np.testing.assert_array_equal(np.asarray(TiffArray(str(ref))[0:13]), a.astype(np.float32))


@pytest.mark.parametrize("dtype", ["uint16", "int16", "float32"])
def test_streaming_writer_reads_back_through_pillow(tmp_path, dtype):
    Image = pytest.importorskip("PIL.Image")
    a = _frames(dtype, T=4)
    p = str(tmp_path / "s.tif")
    _stream(p, a, False, [3, 1])
    with Image.open(p) as im:
        for t in range(4):
            im.seek(t)
            got = np.asarray(im)
            assert got.shape == a.shape[1:]
            np.testing.assert_array_equal(got.astype(a.dtype), a[t])
            assert got.astype(a.dtype).tobytes() == a[t].tobytes()


def test_bigtiff_decision_at_4gib():
    limit = (1 << 32) - (1 << 20)
    h, w = 512, 512
    page = h * w * 4
    n = limit // (page + 256)
    assert not tiff_needs_bigtiff(n, h, w, 4)
    assert tiff_needs_bigtiff(n + 1, h, w, 4)
    assert not tiff_needs_bigtiff(3, 9, 11, 2)


def test_writer_rejects_oversized_classic_and_extra_frames(tmp_path):
    p = str(tmp_path / "x.tif")
    with pytest.raises(ValueError):
        TiffWriter(p, (70000, 128, 128), np.float32, bigtiff=False)
    assert not os.path.exists(p)
    tw = TiffWriter(p, (2, 3, 4), np.uint16)
    with pytest.raises(ValueError):
        tw.write(np.zeros((3, 3, 4), np.uint16))
    with pytest.raises(ValueError):
        tw.write(np.zeros((1, 3, 5), np.uint16))
    tw.abort()


def test_aborted_writer_removes_its_file(tmp_path):
    p = tmp_path / "a.tif"
    with pytest.raises(RuntimeError):
        with TiffWriter(str(p), (5, 3, 4), np.float32) as tw:
            tw.write(np.zeros((2, 3, 4), np.float32))
            assert p.exists()
            raise RuntimeError("midway")
    assert not p.exists()
    tw = TiffWriter(str(p), (5, 3, 4), np.float32)
    tw.write(np.zeros((2, 3, 4), np.float32))
    with pytest.raises(ValueError):
        tw.close()                      # frames missing
    assert not p.exists()


# ---- quantiser -----------------------------------------------------------------------------------------------------
def test_quantize_half_way_saturation_nan():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 65534.5, 65535.4, 65535.6, 1e9, -3.0, -1e9, np.nan, np.inf, -np.inf, 7.49],
                 np.float32)
    np.testing.assert_array_equal(E.quantize(v, "uint16"),
                                  np.array([0, 2, 2, 0, 0, 65534, 65535, 65535, 65535, 0, 0, 0, 65535, 0, 7], np.uint16))
    w = np.array([0.5, 1.5, -2.5, 32766.5, 32767.5, -32768.5, -32769.0, 1e9, -1e9, np.nan, np.inf, -np.inf], np.float32)
    np.testing.assert_array_equal(E.quantize(w, "int16"),
                                  np.array([0, 2, -2, 32766, 32767, -32768, -32768, 32767, -32768, 0, 32767, -32768],
                                           np.int16))
    f = np.array([np.nan, 1.25], np.float32)
    got = E.quantize(f, "float32")
    assert got.dtype == np.float32 and np.isnan(got[0]) and got[1] == 1.25
