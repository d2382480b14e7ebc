"""
Kernel-level tests of the sparse assembly and of the global stage's tile bookkeeping (GPU), every entry point called by name
through the C ABI on tables built from localmd_amd.grid, as the host driver builds them (decomposition.py):

    pmd_csr_count / pmd_csr_fill    against the reference's literal construction (tests.util.reference_sparse_u), bit for bit,
                                    and against the host construction the driver falls back to (_sparse_u)
    pmd_weight_tiles                against float64 u w / cumw; padding exactly +0.0
    pmd_compact_rows                bit-exact copy; everything else of Z untouched
    the launch split at 32 768 tiles of pmd_weight_tiles, pmd_compact_rows and pmd_tiles_truncate
"""
import functools
import zlib

import numpy as np
import pytest
import scipy.sparse

from localmd_amd import grid
from tests.util import reference_sparse_u

pytestmark = pytest.mark.gpu

PMD_ERR_ARG = -2
U32 = 2.0 ** -24     # unit roundoff of fp32

GEOMETRIES = {
    # name: (fov, block, origins covering a pixel along each axis at most)
    "nine_covers": ((33, 47), (20, 20), (3, 3)),        # 1, 2 and 3 covering origins along both axes: pixels under 1 to 9 tiles
    "nonsquare": ((41, 45), (20, 16), (3, 3)),          # last origin of the first axis snapped by one pixel
    "tile_column": ((25, 20), (20, 20), (2, 1)),
    "one_tile": ((20, 20), (20, 20), (1, 1)),
}


def _t():
    import torch

    return torch


def P(t):
    from localmd_amd._lib import ptr

    return ptr(t)


def _dev(ctx, a, dtype=None):
    torch = _t()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ctx.device)


def _bits(a):
    """The bit patterns of a float32 / float64 array (NaN payloads and the sign of zero included)."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


@functools.lru_cache(maxsize=None)
def _geometry(name):
    fov, block, covers = GEOMETRIES[name]
    it1, it2 = grid.tile_origins(fov, block)
    pix, origins = grid.tile_pixel_lists(fov, block, it1, it2)
    bw = grid.block_weight_matrix(block)
    cumw = grid.cumulative_weights(fov, block, origins, bw)
    cov1, cov2 = grid.cover_tables(fov, block, it1, it2)
    n1 = (cov1 >= 0).sum(1)
    n2 = (cov2 >= 0).sum(1)
    # the covers the table promises: every count from 1 to the maximum occurs along both axes
    assert set(n1) == set(range(1, covers[0] + 1)) and set(n2) == set(range(1, covers[1] + 1)), (name, set(n1), set(n2))
    return dict(fov=fov, block=block, it1=it1, it2=it2, pix=pix, origins=origins, bw=bw, cumw=cumw, cov1=cov1, cov2=cov2,
                n_tiles=pix.shape[0], d=block[0] * block[1], covers=np.outer(n1, n2))


def test_geometries_cover_what_they_claim():
    """(33, 47) with 20 x 20 blocks has pixels under 1, 2, 3, 4, 6 and 9 tiles; (41, 45) with 20 x 16 blocks snaps the last
    origin of its first axis by one pixel; (25, 20) is a single tile column; (20, 20) one tile."""
    g = _geometry("nine_covers")
    assert set(np.unique(g["covers"])) == {1, 2, 3, 4, 6, 9}
    g = _geometry("nonsquare")
    assert g["it1"][-1] - g["it1"][-2] == 1 and g["covers"].max() == 9
    g = _geometry("tile_column")
    assert len(g["it2"]) == 1 and len(g["it1"]) == 2
    assert _geometry("one_tile")["n_tiles"] == 1


def _tile_ranks(rng, n, max_rank):
    """Random ranks that include the maximum and, with more than one tile, 0."""
    ranks = rng.integers(0, max_rank + 1, n)
    ranks[0] = max_rank
    if n > 1:
        ranks[n // 2] = 0
    if n > 2:
        ranks[-1] = 1
    return ranks.astype(np.int64)


def _tile_bases(ctx, rng, g, ranks, rpad):
    """Ut (n_tiles, rpad, dpad) float32: random below the rank and inside the tile, NaN in every row at or beyond the rank
    and in every column at or beyond d (neither may be read)."""
    d = g["d"]
    dpad = int(ctx.lib.pmd_tile_dpad(d))
    ut = np.full((g["n_tiles"], rpad, dpad), np.nan, dtype=np.float32)
    for t, rk in enumerate(ranks):
        ut[t, :rk, :d] = rng.standard_normal((rk, d)).astype(np.float32)
    return ut, dpad


def _run_csr(ctx, g, order, K, rpad, ut, ranks, basis_c, tail=16):
    """pmd_csr_count + pmd_csr_fill as _assemble_u calls them.  Returns (row_nnz, indptr, data, indices, zero_count) on the
    host; data / indices carry `tail` sentinel entries (NaN / -1) behind indptr[-1]."""
    torch = _t()
    d1, d2 = g["fov"]
    D = d1 * d2
    offsets = np.concatenate([[0], np.cumsum(ranks)]).astype(np.int64)
    Rt = int(offsets[-1])
    ranks_dev, col_off_dev = _dev(ctx, ranks, np.int32), _dev(ctx, offsets[:-1], np.int32)
    w_dev = _dev(ctx, g["bw"].reshape(-1, order="F"), np.float32)
    inv_dev = _dev(ctx, 1.0 / g["cumw"].reshape(-1), np.float64)
    cov1, cov2 = _dev(ctx, g["cov1"], np.int32), _dev(ctx, g["cov2"], np.int32)
    o1, o2 = _dev(ctx, g["it1"], np.int32), _dev(ctx, g["it2"], np.int32)
    n2 = len(g["it2"])
    order_f = 1 if order == "F" else 0
    ut_dev = _dev(ctx, ut)
    basis_dev = _dev(ctx, basis_c if K > 0 else np.full((1, 1), np.nan, np.float32), np.float32)
    row_nnz = torch.full((D,), -7, dtype=torch.int64, device=ctx.device)
    ctx.call("pmd_csr_count", d1, d2, order_f, P(cov1), P(cov2), n2, P(ranks_dev), K, P(row_nnz))
    indptr = torch.zeros(D + 1, dtype=torch.int64, device=ctx.device)
    indptr[1:] = torch.cumsum(row_nnz, 0)
    nnz = int(indptr[-1].item())
    data = torch.full((nnz + tail,), float("nan"), dtype=torch.float64, device=ctx.device)
    idx = torch.full((nnz + tail,), -1, dtype=torch.int32, device=ctx.device)
    zero = torch.full((1,), 12345, dtype=torch.int32, device=ctx.device)
    args = [d1, d2, order_f, g["block"][0], P(cov1), P(cov2), P(o1), P(o2), n2, P(ranks_dev), P(col_off_dev), P(ut_dev),
            ut.shape[2], P(w_dev), P(inv_dev), P(basis_dev), K, Rt, P(indptr), P(data), P(idx), P(zero)]
    assert ctx.lib.pmd_csr_fill(ctx.handle, *args, 96) == PMD_ERR_ARG      # 96 component rows: not a multiple of 64
    ctx.sync()
    assert torch.isnan(data).all() and int(zero.item()) == 12345, "the rejected call wrote"
    ctx.call("pmd_csr_fill", *args, rpad)
    ctx.sync()
    return row_nnz.cpu().numpy(), indptr.cpu().numpy(), data.cpu().numpy(), idx.cpu().numpy(), int(zero.item())


def _basis_rows(g, order, basis_c):
    """The K basis columns (given by C-order pixel, as the device holds them) by output row."""
    d1, d2 = g["fov"]
    fov_ids = np.arange(d1 * d2).reshape((d1, d2), order=order)
    rows = np.empty_like(basis_c)
    rows[fov_ids.reshape(-1)] = basis_c
    return rows


@pytest.mark.parametrize("rpad", [64, 128])
@pytest.mark.parametrize("K", [0, 1, 3])
@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_csr_count_and_fill_are_bitwise_the_reference_construction(gpu_ctx, name, order, K, rpad):
    """pmd_csr_count / pmd_csr_fill against the reference's literal construction with the K basis columns appended: row
    counts, column indices and values bit for bit (a value is two float64 multiplications), indices strictly ascending
    within a row, nothing written behind indptr[-1], no zero counted.  rpad = 128 with ranks up to 70."""
    ctx = gpu_ctx
    g = _geometry(name)
    d1, d2 = g["fov"]
    D = d1 * d2
    rng = np.random.default_rng(zlib.crc32(f"{name}/{order}/{K}/{rpad}".encode()))
    ranks = _tile_ranks(rng, g["n_tiles"], 54 if rpad == 64 else 70)
    ut, _ = _tile_bases(ctx, rng, g, ranks, rpad)
    basis_c = rng.standard_normal((D, max(K, 1))).astype(np.float32)[:, :K]
    row_nnz, indptr, data, idx, zeros = _run_csr(ctx, g, order, K, rpad, ut, ranks, basis_c)
    ref = reference_sparse_u(ut, ranks, g["origins"], g["fov"], g["block"], order, g["bw"])
    if K > 0:
        ref = scipy.sparse.hstack([ref, scipy.sparse.csr_matrix(_basis_rows(g, order, basis_c).astype(np.float64))]).tocsr()
        ref.sort_indices()
    nnz = int(indptr[-1])
    np.testing.assert_array_equal(row_nnz, np.diff(ref.indptr))
    assert nnz == ref.nnz
    np.testing.assert_array_equal(idx[:nnz], ref.indices)
    np.testing.assert_array_equal(_bits(data[:nnz]), _bits(ref.data))
    inner = np.ones(nnz, dtype=bool)
    inner[indptr[1:-1][indptr[1:-1] < nnz]] = False       # first entry of a row
    assert np.all(np.diff(idx[:nnz])[inner[1:]] > 0), "indices not strictly ascending within a row"
    assert np.all(np.isnan(data[nnz:])) and np.all(idx[nnz:] == -1), "written behind indptr[-1]"
    assert zeros == 0


@pytest.mark.parametrize("rpad", [64, 128])
@pytest.mark.parametrize("K", [0, 3])
@pytest.mark.parametrize("order", ["F", "C"])
def test_csr_zero_counter_and_host_construction(gpu_ctx, order, K, rpad):
    """The zero counter of pmd_csr_fill decides whether the driver keeps the device CSR or rebuilds U on the host
    (_assemble_u): with z1 exact zeros planted inside kept components (one at a pixel under nine tiles) and z2 in the basis it
    counts z1 + z2 - zeros in rows at or beyond a tile's rank are not counted - and the host construction (_sparse_u with
    the basis stacked on, as in the host branch) equals the device CSR without its exact zeros, bit for bit."""
    from localmd_amd.decomposition import _sparse_u

    ctx = gpu_ctx
    g = _geometry("nine_covers")
    d1, d2 = g["fov"]
    b1, b2 = g["block"]
    D, d, n = d1 * d2, g["d"], g["n_tiles"]
    rng = np.random.default_rng(zlib.crc32(f"zeros/{order}/{K}/{rpad}".encode()))
    ranks = rng.integers(1, 7 if rpad == 64 else 71, n).astype(np.int64)
    ranks[0] = 0
    ut, _ = _tile_bases(ctx, rng, g, ranks, rpad)
    # a pixel under nine tiles, and the last of its tiles
    i9, j9 = [int(v[0]) for v in np.nonzero(g["covers"] == 9)]
    t9 = max(t for t, (k, j) in enumerate(g["origins"]) if k <= i9 < k + b1 and j <= j9 < j + b2)
    k9, jo9 = g["origins"][t9]
    planted = {(t9, int(ranks[t9]) - 1, (i9 - k9) + b1 * (j9 - jo9))}
    while len(planted) < 5:
        t = int(rng.integers(1, n))
        planted.add((t, int(rng.integers(0, ranks[t])), int(rng.integers(0, d))))
    for t, c, q in planted:
        ut[t, c, q] = 0.0
    for t in range(n):                      # zeros the kernel must not see: component rows at or beyond the rank
        ut[t, ranks[t]:ranks[t] + 2, ::7] = 0.0
    basis_c = rng.standard_normal((D, max(K, 1))).astype(np.float32)[:, :K]
    z2 = 0
    if K > 0:
        basis_c[i9 * d2 + j9, 1] = 0.0
        basis_c[5, K - 1] = 0.0
        z2 = 2
    row_nnz, indptr, data, idx, zeros = _run_csr(ctx, g, order, K, rpad, ut, ranks, basis_c)
    assert zeros == len(planted) + z2, (zeros, len(planted), z2)
    nnz = int(indptr[-1])
    assert int((data[:nnz] == 0).sum()) == zeros
    Rt = int(ranks.sum())
    R = Rt + (K if K > 0 else 1)
    dev = scipy.sparse.csr_matrix((data[:nnz], idx[:nnz], indptr), shape=(D, R))
    dense_dev = dev.toarray()
    dev.eliminate_zeros()
    dev.sort_indices()
    # the host branch of _assemble_u
    fov_ids = np.arange(D).reshape((d1, d2), order=order)
    pix_f = fov_ids.reshape(-1)[g["pix"]]
    inv_rows = np.zeros(D)
    inv_rows[fov_ids.reshape(-1)] = 1.0 / g["cumw"].reshape(-1)
    u_local, _ = _sparse_u(ut, ranks, pix_f, g["bw"], inv_rows, D)
    right = scipy.sparse.coo_matrix(_basis_rows(g, order, basis_c)) if K > 0 else scipy.sparse.coo_matrix((D, 1), dtype=np.float32)
    host = scipy.sparse.hstack([u_local, right]).tocsr()
    host.sort_indices()
    assert host.shape == dev.shape
    np.testing.assert_array_equal(_bits(host.toarray().astype(np.float64)), _bits(dense_dev))
    np.testing.assert_array_equal(host.indptr, dev.indptr)
    np.testing.assert_array_equal(host.indices, dev.indices)
    np.testing.assert_array_equal(_bits(host.data.astype(np.float64)), _bits(dev.data))


# ------------------------------------------------------------------------------------------------------------------
# pmd_weight_tiles

def _check_weighted(uw, ut, pix, w, cumw, ranks, d):
    """uw against float64 ut w / cumw: below the rank and inside the tile within 4 2^-24 relative (two fp32 roundings of at
    most one ulp each); every other entry exactly +0.0."""
    for t in range(ut.shape[0]):
        rk = int(ranks[t])
        ref = ut[t, :rk, :d].astype(np.float64) * w[None, :].astype(np.float64) / cumw[pix[t]][None, :].astype(np.float64)
        got = uw[t, :rk, :d].astype(np.float64)
        err = np.abs(got - ref)
        assert np.all(err <= 4 * U32 * np.abs(ref)), (t, float((err / np.abs(ref)).max()))
        pad = np.ones(uw.shape[1:], dtype=bool)
        pad[:rk, :d] = False
        assert np.all(_bits(uw[t])[pad] == 0), ("padding is not +0.0", t)


@pytest.mark.parametrize("fov,block", [((23, 27), (10, 10)), ((33, 47), (20, 20)), ((41, 45), (20, 16))])
def test_weight_tiles_matches_float64_and_zeroes_the_padding(gpu_ctx, fov, block):
    """pmd_weight_tiles on the virtual-tile layout (blocks of 64 component rows, two per tile: ranks 0, 1, 63 and 64 among
    the blocks), d = 100, 400 and 320 at their pmd_tile_dpad (256, 400, 400); Ut holds NaN in every row at or beyond the rank and every
    column at or beyond d; a guard block behind the last one stays untouched."""
    torch = _t()
    ctx = gpu_ctx
    it1, it2 = grid.tile_origins(fov, block)
    pix, origins = grid.tile_pixel_lists(fov, block, it1, it2)
    bw = grid.block_weight_matrix(block)
    cumw = grid.cumulative_weights(fov, block, origins, bw).reshape(-1).astype(np.float32)
    w = bw.reshape(-1, order="F").astype(np.float32)
    d = block[0] * block[1]
    dpad = int(ctx.lib.pmd_tile_dpad(d))
    nvt = 2
    cycle = [0, 1, 63, 64, 65, 127, 128, 20]
    tile_ranks = np.array([cycle[i % len(cycle)] for i in range(len(origins))])
    ranks = np.clip(tile_ranks[:, None] - 64 * np.arange(nvt)[None, :], 0, 64).reshape(-1)
    assert {0, 1, 63, 64} <= set(ranks.tolist())
    pix_v = np.repeat(pix, nvt, axis=0)
    n = len(ranks)
    rng = np.random.default_rng(d)
    ut = np.full((n, 64, dpad), np.nan, dtype=np.float32)
    for t in range(n):
        ut[t, :ranks[t], :d] = rng.standard_normal((ranks[t], d)).astype(np.float32)
    uw = torch.full((n + 1, 64, dpad), 7.0, device=ctx.device)
    # (named: a tensor must outlive the asynchronous call that reads it)
    ut_dev, pix_dev, w_dev, cumw_dev, ranks_dev = _dev(ctx, ut), _dev(ctx, pix_v, np.int32), _dev(ctx, w), _dev(ctx, cumw), _dev(ctx, ranks, np.int32)
    ctx.call("pmd_weight_tiles", P(ut_dev), dpad, P(pix_dev), d, P(w_dev), P(cumw_dev), P(ranks_dev), P(uw), n)
    ctx.sync()
    uw = uw.cpu().numpy()
    _check_weighted(uw[:n], ut, pix_v, w, cumw, ranks, d)
    assert np.all(uw[n] == 7.0), "guard block written"


# ------------------------------------------------------------------------------------------------------------------
# pmd_compact_rows

@pytest.mark.parametrize("T", [1, 77, 4100])
def test_compact_rows_is_a_bitwise_copy_and_touches_nothing_else(gpu_ctx, T):
    """pmd_compact_rows with ranks 0, 1, 33 and 64, T = 4100 beyond one sweep of its 16 x 256 grid, ldz > T and gaps between
    the tiles' rows of Z: Z, pre-filled with a NaN sentinel, holds Out's rows below the rank bit for bit and the sentinel
    everywhere else (rows not named by (col_off, ranks), columns at or beyond T).  Then the call on a tile sub-range, as
    _right_matrix and _ZBuilder._project_tiles make it."""
    torch = _t()
    ctx = gpu_ctx
    ranks = np.array([64, 0, 1, 33, 64, 33, 1, 0, 64], dtype=np.int64)
    n = len(ranks)
    ldo, ldz = T + 5, T + 3
    off = np.concatenate([[1], 1 + np.cumsum(ranks + 2)]).astype(np.int64)      # two rows of Z between the tiles, one in front
    rows = int(off[-1]) + 3
    g = torch.Generator(device=ctx.device).manual_seed(T)
    out = torch.randn((n, 64, ldo), device=ctx.device, generator=g)
    out[:, :, T:] = float("inf")
    for t in range(n):
        out[t, int(ranks[t]):] = float("inf")
    ranks_dev, off_dev = _dev(ctx, ranks, np.int32), _dev(ctx, off[:-1], np.int32)
    for t_lo in (0, 4):
        z = torch.full((rows, ldz), float("nan"), device=ctx.device)
        expect = z.clone()
        for t in range(t_lo, n):
            rk = int(ranks[t])
            expect[off[t]:off[t] + rk, :T] = out[t, :rk, :T]
        ctx.call("pmd_compact_rows", P(out[t_lo:]), ldo, P(off_dev[t_lo:]), P(ranks_dev[t_lo:]), T, P(z), ldz, n - t_lo)
        ctx.sync()
        assert torch.equal(z.view(torch.int32), expect.view(torch.int32)), (T, t_lo)


# ------------------------------------------------------------------------------------------------------------------
# the launch split at 32 768 tiles

N_SPLIT = 32768 + 3
SPLIT_TILES = [0, 32766, 32767, 32768, 32769, 32770]
SPLIT_RANKS = [64, 1, 33, 0, 64, 17]


def _need_memory(ctx):
    torch = _t()
    free, _ = torch.cuda.mem_get_info(ctx.device)
    if free < 4 * 2 ** 30:
        pytest.skip("less than 4 GB of device memory free: the 32 771-tile arrays do not fit")


def _split_ranks(ctx, seed):
    torch = _t()
    g = torch.Generator(device=ctx.device).manual_seed(seed)
    ranks = torch.randint(0, 65, (N_SPLIT,), device=ctx.device, generator=g, dtype=torch.int32)
    ranks[SPLIT_TILES] = torch.tensor(SPLIT_RANKS, dtype=torch.int32, device=ctx.device)
    return ranks, g


def test_weight_tiles_beyond_32768_tiles(gpu_ctx):
    """pmd_weight_tiles over 32 771 blocks (two launches), d = 40 at leading dimension 64, inputs generated on the device:
    blocks 0 and 32 766 ... 32 770 against float64 as above, the guard block untouched."""
    torch = _t()
    ctx = gpu_ctx
    _need_memory(ctx)
    d, dpad, n_pix = 40, 64, 5000
    ranks, g = _split_ranks(ctx, 1)
    ut = torch.randn((N_SPLIT, 64, dpad), device=ctx.device, generator=g)
    ut[:, :, d:] = float("nan")
    ut.masked_fill_(torch.arange(64, device=ctx.device)[None, :, None] >= ranks[:, None, None], float("nan"))
    pix = torch.randint(0, n_pix, (N_SPLIT, d), device=ctx.device, generator=g, dtype=torch.int32)
    w = torch.randint(1, 11, (d,), device=ctx.device, generator=g).float()
    cumw = torch.randint(1, 40, (n_pix,), device=ctx.device, generator=g).float()
    uw = torch.full((N_SPLIT + 1, 64, dpad), 7.0, device=ctx.device)
    ctx.call("pmd_weight_tiles", P(ut), dpad, P(pix), d, P(w), P(cumw), P(ranks), P(uw), N_SPLIT)
    ctx.sync()
    sel = torch.tensor(SPLIT_TILES, device=ctx.device)
    _check_weighted(uw[sel].cpu().numpy(), ut[sel].cpu().numpy(), pix[sel].cpu().numpy(), w.cpu().numpy(), cumw.cpu().numpy(),
                    SPLIT_RANKS, d)
    assert bool((uw[N_SPLIT] == 7.0).all()), "guard block written"


def test_compact_rows_beyond_32768_tiles(gpu_ctx):
    """pmd_compact_rows over 32 771 tiles (two launches, the second with its own part of col_off and ranks): the rows of
    tiles 0 and 32 766 ... 32 770 are Out's bit for bit, their columns at or beyond T and the guard rows behind the last
    tile keep the sentinel."""
    torch = _t()
    ctx = gpu_ctx
    _need_memory(ctx)
    T, ldo, ldz = 5, 8, 6
    ranks, g = _split_ranks(ctx, 2)
    out = torch.randn((N_SPLIT, 64, ldo), device=ctx.device, generator=g)
    off = (torch.cumsum(ranks, 0) - ranks).to(torch.int32)
    Rt = int(ranks.sum().item())
    z = torch.full((Rt + 4, ldz), float("nan"), device=ctx.device)
    ctx.call("pmd_compact_rows", P(out), ldo, P(off), P(ranks), T, P(z), ldz, N_SPLIT)
    ctx.sync()
    off_h = off[SPLIT_TILES].cpu().numpy()
    for t, rk, o in zip(SPLIT_TILES, SPLIT_RANKS, off_h):
        got = z[int(o):int(o) + rk].cpu().numpy()
        np.testing.assert_array_equal(_bits(got[:, :T]), _bits(out[t, :rk, :T].cpu().numpy()), err_msg=f"tile {t}")
        assert np.all(np.isnan(got[:, T:])), t
    assert int(off_h[-1]) + SPLIT_RANKS[-1] == Rt
    assert bool(torch.isnan(z[Rt:]).all()), "guard rows written"


def test_tiles_truncate_beyond_32768_tiles(gpu_ctx):
    """pmd_tiles_truncate over 32 771 tiles of 64 rows at leading dimension 16: in tiles 0 and 32 766 ... 32 770 the rows
    below the count are unchanged bit for bit, the rows from it on exactly +0.0; the guard tile is untouched."""
    torch = _t()
    ctx = gpu_ctx
    _need_memory(ctx)
    ld = 16
    counts, g = _split_ranks(ctx, 3)
    u = torch.randn((N_SPLIT + 1, 64, ld), device=ctx.device, generator=g)
    u[:, 40:, 3] = float("nan")
    sel = torch.tensor(SPLIT_TILES + [N_SPLIT], device=ctx.device)
    before = u[sel].cpu().numpy()
    ctx.call("pmd_tiles_truncate", P(u), ld, P(counts), N_SPLIT, 64)
    ctx.sync()
    after = u[sel].cpu().numpy()
    for i, k in enumerate(SPLIT_RANKS):
        np.testing.assert_array_equal(_bits(after[i, :k]), _bits(before[i, :k]))
        assert np.all(_bits(after[i, k:]) == 0), SPLIT_TILES[i]
    np.testing.assert_array_equal(_bits(after[-1]), _bits(before[-1]), err_msg="guard tile written")
