"""Host checks of tests/tile_gemm_ref.py: the case tables of the tile contraction tests reach every kernel instantiation
that pmd_launch_tile_* can choose, the exact cases stay exact, and the references are the contractions they claim to be."""
import numpy as np

from tests import tile_gemm_ref as R


def _kinds(cases, kind):
    return [c for c in cases if kind in c.kinds]


def _atx_routes(cases):
    out = set()
    for c in cases:
        for rank in (c.ranks if c.ranks is not None else (None,)):
            out.add(R.atx_route(c, rank))
    return out


def test_exact_cases_stay_below_2_to_24():
    cases = R.atx_cases() + R.xbt_cases() + R.gram_cases() + R.rowmix_cases()
    exact = _kinds(cases, "exact")
    assert len(exact) > 1000
    worst = max(R.exact_magnitude(c) for c in exact)
    assert worst == 49 * 2500 and worst < R.EXACT_LIMIT
    assert max(R.exact_magnitude(c) for c in exact if isinstance(c, R.RowmixCase)) == 49 * 64
    # the integers themselves and every partial sum are fp32 numbers
    assert np.float32(worst) == worst and np.float32(R.EXACT_LIMIT - 1) == R.EXACT_LIMIT - 1


def test_exact_cases_reach_every_atx_route():
    exact = _kinds(R.atx_cases(), "exact")
    assert _atx_routes(exact) == {
        "tile_atx_kernel<16,1,2>", "tile_atx_kernel<32,1,1>",        # bare variants
        "tile_atx_kernel<25,1,1>",                                   # register-staged
        "tile_atx_dma_kernel<25>", "tile_atx_dma_kernel<25>:half",   # LDS-DMA ring, full and half tiles
        "tile_atx_kernel<25,2,1>", "tile_atx_kernel<32,2,1>", "tile_atx_kernel<8,8,1,1>"}
    # the register-staged kernel by shape (short rows) and by switch
    staged = [c for c in exact if R.atx_route(c) == "tile_atx_kernel<25,1,1>"]
    assert {(c.env, c.ld) for c in staged} >= {("default", "r32"), ("atx_dma0", "time")}
    # the one-row-tile kernel below and at the variant's upper end
    assert {c.d for c in exact if R.atx_route(c) == "tile_atx_kernel<8,8,1,1>"} == {1000, 1024}
    assert {c.rows for c in exact if c.d == 1024 and R.atx_route(c) == "tile_atx_kernel<32,2,1>"} >= {0, 17}
    # grid-level K slices
    kz = {R.atx_launch(c.d, c.T, c.slices)[0] for c in exact}
    assert {1, 2} <= kz and max(kz) >= 3
    # the DMA ring with 1, 2, 3, 4 and more chunks per workgroup; a last workgroup shorter than the others
    ring = [R.atx_slice_chunks(c.T, c.slices) for c in exact if R.atx_route(c).startswith("tile_atx_dma")]
    assert {n for chunks in ring for n in chunks} >= {1, 2, 3, 4, 6}
    assert any(len(set(chunks)) > 1 for chunks in ring)
    # both sides of every variant boundary
    for lo in (256, 400, 512, 800, 1024):
        assert R.atx_route(_one(exact, d=lo)) != R.atx_route(_one(exact, d=lo + 1)) or lo == 1024
    assert R.atx_launch(1024, 32, 1)[0] == 1 and R.atx_launch(1025, 32, 1)[0] == 2
    # the XCD remapping (>= 64 tiles) with one and with two K slices, tile counts that are no multiple of 8
    many = [c for c in exact if c.n_tiles >= 64]
    assert {(c.n_tiles % 8 != 0, R.atx_launch(c.d, c.T, c.slices)[0]) for c in many} >= {(True, 1), (True, 2), (False, 1), (False, 2)}
    # argument forms and entry points
    assert {c.form for c in exact} == {"pix", "tight", "row0", "shared_a"}
    assert {c.entry for c in exact} == {"pmdk_tile_atx", "pmdk_tile_atx_rows", "pmd_tiles_project", "pmd_tiles_project_ranked"}


def _one(cases, **want):
    return next(c for c in cases if all(getattr(c, k) == v for k, v in want.items()) and c.form == "pix" and c.ld == "time" and
                c.env == "default" and c.rows == 0)


def test_exact_cases_reach_every_xbt_route():
    exact = _kinds(R.xbt_cases(), "exact")
    reached = {(R.route_of_xbt(c.d), R.xbt_launch(c.d, c.T, c.slices)[3]) for c in exact}
    assert reached == {("tile_xbt_lds_kernel<1>", 1), ("tile_xbt_lds_kernel<2>", 1), ("tile_xbt_lds_kernel<4>", 1),
                       ("tile_xbt_lds_kernel<7>", 1), ("tile_xbt_lds_kernel<7>", 2), ("tile_xbt_lds_kernel<7>", 3)}
    # slices without work (cleared by the launcher), with few and with many tiles; odd and even group counts per slice
    idle = [c for c in exact if c.slices > 1 and R.xbt_launch(c.d, c.T, c.slices)[1] < c.slices]
    assert {c.T for c in idle} >= {1, 16, 17, 33, 48, 80, 133, 144} and any(c.n_tiles >= 64 for c in idle)
    assert {R.xbt_launch(c.d, c.T, c.slices)[2] for c in exact} >= {1, 2, 3, 5, 16, 63}
    assert {c.form for c in exact} == {"pix", "row0", "shared_b", "stride0"}


def test_exact_cases_reach_every_gram_route():
    exact = _kinds(R.gram_cases(), "exact")
    assert {R.gram_route(c) for c in exact} == {"tile_gram_mfma_kernel", "tile_gram_kernel"}
    scalar = [c for c in exact if R.gram_route(c) == "tile_gram_kernel"]
    assert any(c.env == "gram0" for c in scalar)                                    # by switch
    assert any(c.env == "default" and c.ld % 4 and not c.offset for c in scalar)    # by leading dimension
    assert any(c.env == "default" and c.ld % 4 == 0 and c.ld >= 16 and c.offset for c in scalar)   # by alignment
    mfma = [c for c in exact if R.gram_route(c) == "tile_gram_mfma_kernel"]
    assert any(c.len == c.ld for c in mfma), "the clamp of the last quad at the row's end"
    assert any(R.gram_chunk(c.len, c.slices) * (c.slices - 2) >= c.len for c in mfma), "two empty slices"


def test_exact_cases_reach_every_rowmix_route():
    exact = _kinds(R.rowmix_cases(), "exact")
    assert {R.rowmix_route(c) for c in exact} == {"tile_rowmix_mfma4_kernel", "tile_rowmix_mfma_kernel", "tile_rowmix_kernel<4>",
                                                  "tile_rowmix_kernel<32>", "tile_rowmix_kernel<64>"}
    assert max(R.rowmix_passes(c.n_tiles) for c in exact) == 2
    by_count = {c.n_tiles: R.rowmix_route(c) for c in R.ROWMIX_MANY}
    assert by_count == {8191: "tile_rowmix_mfma_kernel", 8192: "tile_rowmix_mfma4_kernel", 32769: "tile_rowmix_mfma4_kernel"}
    # the 64-position form asked for by switch gives way on rows that are not 16-byte aligned and on len < 4
    asked = [c for c in exact if c.env == "rowmix64" and c.n_out > 4]
    back = [c for c in asked if R.rowmix_route(c) == "tile_rowmix_mfma_kernel"]
    assert any(c.ld_in % 4 for c in back) and any(c.len < 4 and c.ld_in % 4 == 0 for c in back)
    assert any(R.rowmix_route(c) == "tile_rowmix_mfma4_kernel" and c.len % 4 for c in asked), "the partial last quad"
    for env in R.ROWMIX_ENVS:
        mine = [c for c in exact if c.env == env]
        assert {c.inplace for c in mine} == {True, False} and {c.n_stride for c in mine} >= {0, 4096}
        assert any(c.ld_in != c.ld_out for c in mine)


def test_rounded_cases_reach_every_family():
    assert {R.atx_route(c).split("<")[0] for c in _kinds(R.atx_cases(), "rounded")} == {"tile_atx_kernel", "tile_atx_dma_kernel"}
    assert any(R.atx_launch(c.d, c.T, c.slices)[0] > 1 for c in _kinds(R.atx_cases(), "rounded"))
    assert {R.route_of_xbt(c.d) for c in _kinds(R.xbt_cases(), "rounded")} == {"tile_xbt_lds_kernel<%d>" % m for m in (1, 2, 4, 7)}
    assert {R.gram_route(c) for c in _kinds(R.gram_cases(), "rounded")} == {"tile_gram_mfma_kernel", "tile_gram_kernel"}
    assert {R.rowmix_route(c) for c in _kinds(R.rowmix_cases(), "rounded")} == {
        "tile_rowmix_mfma4_kernel", "tile_rowmix_mfma_kernel", "tile_rowmix_kernel<4>", "tile_rowmix_kernel<32>", "tile_rowmix_kernel<64>"}


def test_shape_restatements():
    assert [R.time_ld(t) for t in (1, 64, 65, 1000)] == [128, 128, 192, 1088]
    assert [R.tile_dpad(d) for d in (1, 256, 257, 400, 401, 512, 513, 800, 801, 1024, 1025, 2049)] == [
        256, 256, 400, 400, 512, 512, 800, 800, 1024, 1024, 2048, 3072]
    # pmd_time_ld always leaves the LDS-DMA kernel its two spare chunks
    assert all(R.time_ld(T) >= 32 * (R.ceil_div(T, 32) + 2) for T in range(1, 3000))
    assert R.atx_launch(300, 161, 3) == (1, 3, 2) and R.atx_slice_chunks(129, 2) == [3, 2]
    assert R.xbt_launch(449, 133, 4) == (7, 3, 3, 2) and R.xbt_launch(1024, 1, 4) == (7, 1, 1, 3)
    assert R.gram_chunk(33, 4) == 32 and R.gram_chunk(1234, 7) == 192


def test_references_against_einsum():
    rng = np.random.default_rng(0)
    A, X = rng.standard_normal((2, 64, 5)), rng.standard_normal((2, 5, 7))
    B, In, N = rng.standard_normal((2, 64, 7)), rng.standard_normal((2, 64, 9)), rng.standard_normal((2, 6, 4))
    for (got, gabs), spec, ops in ((R.ref_atx(A, X), "ncq,nqt->nct", (A, X)), (R.ref_xbt(B, X), "nct,nqt->ncq", (B, X)),
                                   (R.ref_gram(In), "nix,njx->nij", (In, In)), (R.ref_rowmix(N, In[:, :6]), "npc,npx->ncx", (N, In[:, :6]))):
        np.testing.assert_allclose(got, np.einsum(spec, *ops), rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(gabs, np.einsum(spec, *[np.abs(o) for o in ops]), rtol=1e-13, atol=1e-13)
        assert np.all(np.abs(got) <= gabs * (1 + 1e-12))
    # float32 operands are taken to float64 before anything is multiplied
    a32 = np.full((1, 1, 3), 1 + 2.0 ** -23, dtype=np.float32)
    assert R.ref_gram(a32)[0][0, 0, 0] == 3 * (1 + 2.0 ** -23) ** 2


def test_bound_and_data():
    assert R.any_order_bound(100, R.U32, 2.0) == 108 * 2.0 ** -24 * 2.0
    rng = np.random.default_rng(1)
    e = R.exact_data(rng, (4, 64, 100))
    assert e.dtype == np.float32 and np.array_equal(e, np.round(e)) and e.min() == -7 and e.max() == 7
    assert R.exact_data(rng, (3, 3), np.float64).dtype == np.float64
    r = R.rounded_data(rng, (2, 64, 500), decades=True)
    rms = np.sqrt((r.astype(np.float64) ** 2).mean(axis=(0, 2)))
    assert r.dtype == np.float32 and 0.8 < rms[0] < 1.2 and 800 < rms[-1] < 1200
