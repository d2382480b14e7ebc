"""
Kernel-level tests of the global stage's R > frames route (GPU): every entry point of the chain

    pmd_gram_u / pmd_gram_blocks -> pmd_gram_apply -> pmd_gram_mtgm -> pmd_chol_inverse (or pmd_orthogonalize_factored)
    -> pmd_psvd_vp_gram / pmd_psvd_finish / pmd_projected_svd_factored

called by name through the C ABI on tile bookkeeping built as the host driver builds it (decomposition.py), and compared with
a float64 reference of the same operation on the same fp32 inputs.  Large float64 references are formed on the device in row
chunks.  A test that fails here names the kernel and says by how much it is off.
"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

from localmd_amd import grid
from tests.util import context_under

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24     # unit roundoff of fp32


def _t():
    import torch

    return torch


def P(t):
    from localmd_amd._lib import ptr

    return ptr(t)


def _i32(ctx, a):
    torch = _t()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(ctx.device)


def _fresh_ctx(split):
    """A Context of its own: PMD_GEMM_SPLIT, like every route switch, is read when a context is created."""
    return context_under({"PMD_GEMM_SPLIT": None if split else "0"})


def _profiled(ctx, fn):
    ctx.profile_enable(True)
    try:
        fn()
        ctx.sync()
        return ctx.profile_summary()
    finally:
        ctx.profile_enable(False)


def _mtgm64(torch, M, GM, rows, m, chunk=32768):
    """float64 M[:rows, :m]^T GM[:rows, :m] on the device, in row chunks."""
    acc = torch.zeros((m, m), dtype=torch.float64, device=M.device)
    for r0 in range(0, rows, chunk):
        r1 = min(rows, r0 + chunk)
        acc += M[r0:r1, :m].double().T @ GM[r0:r1, :m].double()
    return acc


def _block_errors(Cg, C64, m, bs):
    """Relative Frobenius error of every row block C[i0:i0+bs, 0:i0+bs] (the part pmd_gram_mtgm writes)."""
    out = []
    for i0 in range(0, m, bs):
        i1 = min(m, i0 + bs)
        ref = C64[i0:i1, :i1]
        out.append(float(((Cg[i0:i1, :i1].double() - ref).norm() / ref.norm()).item()))
    return out


def _mtgm_block_size(m):
    # pmd_gram_mtgm's row blocks at the default of five (chol.hip)
    return max(256, ((m + 4) // 5 + 255) // 256 * 256)


# ------------------------------------------------------------------------------------------------------------------
# tile bookkeeping as decomposition.py builds it

LAYOUTS = {
    # name: (fov, block, tile ranks cycled over the tiles, tile rows rpad = 64 nvt)
    "grid70x80": ((70, 80), (10, 10), [0, 1, 15, 16, 17, 32, 33, 48, 64], 1),
    "snapped73x82": ((73, 82), (10, 10), [64, 33, 0, 17, 48, 1, 16, 32, 15], 1),    # last tiles snapped to the edges
    "virtual": ((43, 52), (10, 10), [118, 0, 64, 65, 1, 100, 17, 33, 127], 2),    # max_components > 54: two virtual tiles
    "headline": ((130, 130), (10, 10), [20], 1),                                  # 625 tiles of rank 20: Rt = 12 500
}


@functools.lru_cache(maxsize=2)
def _layout(name, K, cap=64):
    """Device tables and the dense float64 U (D x (Rt + K)) of a layout; tile ranks capped at `cap` (max_rank buckets)."""
    torch = _t()
    fov, block, rank_cycle, nvt = LAYOUTS[name]
    d1, d2 = fov
    b1, b2 = block
    D = d1 * d2
    it1, it2 = grid.tile_origins(fov, block)
    pix, origins = grid.tile_pixel_lists(fov, block, it1, it2)
    pairs = grid.overlap_pairs(origins, block)
    n_real = len(origins)
    tile_ranks = np.array([rank_cycle[i % len(rank_cycle)] for i in range(n_real)], dtype=np.int64)
    tile_ranks = np.minimum(tile_ranks, cap * nvt)
    d = b1 * b2
    dpad = (d + 63) // 64 * 64
    rng = np.random.default_rng(zlib.crc32(f"{name}/{K}/{cap}".encode()))
    Ut = rng.standard_normal((n_real, 64 * nvt, dpad)).astype(np.float32)
    Ut[:, :, d:] = 0.0
    for t in range(n_real):
        Ut[t, tile_ranks[t]:, :] = 0.0
    # virtual tiles (decomposition.py: blocks of 64 component rows of the same pixels)
    ranks = np.clip(tile_ranks[:, None] - 64 * np.arange(nvt)[None, :], 0, 64).reshape(-1) if nvt > 1 else tile_ranks
    n_tiles = n_real * nvt
    Uw = Ut.reshape(n_tiles, 64, dpad)
    pix_v = np.repeat(pix, nvt, axis=0)
    origins_v = np.repeat(np.asarray(origins), nvt, axis=0)
    pairs_v = grid.virtual_pairs(pairs, nvt)
    col_off = np.concatenate([[0], np.cumsum(ranks)]).astype(np.int64)
    Rt = int(col_off[-1])
    basis = rng.standard_normal((D, max(K, 1))).astype(np.float32)[:, :K] if K > 0 else np.zeros((D, 1), np.float32)
    basis = np.ascontiguousarray(basis)
    # dense U: column col_off[t] + c of virtual tile t holds Uw[t][c][q] at FOV pixel pix[t][q]
    U = np.zeros((D, Rt + K), dtype=np.float64)
    for t in range(n_tiles):
        r = int(ranks[t])
        if r:
            U[pix_v[t], col_off[t]:col_off[t] + r] = Uw[t, :r, :d].T.astype(np.float64)
    if K > 0:
        U[:, Rt:] = basis.astype(np.float64)
    Ud = torch.from_numpy(U).to(torch.device("cuda", 0))
    G64 = (Ud.T @ Ud).cpu().numpy()
    Ga = (Ud.abs().T @ Ud.abs()).cpu().numpy()      # sum of |terms| of every entry
    del Ud
    dev = torch.device("cuda", 0)
    return dict(
        n_tiles=n_tiles, Rt=Rt, K=K, D=D, b1=b1, b2=b2, dpad=dpad, ranks=ranks, col_off=col_off, pairs=pairs_v, G64=G64, Ga=Ga,
        Uw=torch.from_numpy(np.ascontiguousarray(Uw)).to(dev), pix=torch.from_numpy(np.ascontiguousarray(pix_v)).to(dev),
        pairs_dev=torch.from_numpy(np.ascontiguousarray(pairs_v, dtype=np.int32)).to(dev),
        origins=torch.from_numpy(np.ascontiguousarray(origins_v, dtype=np.int32)).to(dev),
        col_off_dev=torch.from_numpy(col_off[:-1].astype(np.int32)).to(dev),
        ranks_dev=torch.from_numpy(ranks.astype(np.int32)).to(dev), basis=torch.from_numpy(basis).to(dev))


def _gram_blocks(ctx, L, ldgs=None):
    torch = _t()
    K, n_tiles, Rt = L["K"], L["n_tiles"], L["Rt"]
    Rc = Rt + K
    ldgs = Rc if ldgs is None else ldgs
    n_pairs = L["pairs"].shape[0]
    gblk = torch.full((n_pairs, 64, 64), float("nan"), device=ctx.device)
    gbg = torch.full((max(1, (K + 63) // 64) * n_tiles, 64, 64), float("nan"), device=ctx.device)
    gstrip = torch.full((max(K, 1), ldgs), float("nan"), device=ctx.device)
    ctx.call("pmd_gram_blocks", P(L["Uw"]), L["dpad"], L["b1"], L["b2"], P(L["pix"]), P(L["pairs_dev"]), n_pairs, P(L["origins"]),
             P(L["col_off_dev"]), P(L["ranks_dev"]), n_tiles, Rt, P(L["basis"]), L["D"], K, P(gblk), P(gbg), P(gstrip), ldgs)
    ctx.sync()
    return gblk, gbg, gstrip


def _within_one_ulp(got, ref, absterms):
    """|got - ref| <= one fp32 ulp of ref, with a floor of 1e-12 sum|terms| for entries that cancel."""
    tol = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 1e-12 * absterms
    return np.abs(got.astype(np.float64) - ref) <= tol


@pytest.mark.parametrize("K", [0, 3, 64, 70, 130])
@pytest.mark.parametrize("name", ["grid70x80", "snapped73x82", "virtual"])
def test_gram_u_and_blocks_match_float64(gpu_ctx, name, K):
    """pmd_gram_u (dense G) and pmd_gram_blocks (Gblk / Gbg / Gstrip) sum in fp64 and round once: every entry within one fp32
    ulp of the float64 U^T U, tile x tile, tile x background and background x background; block entries beyond the ranks
    exactly zero; and the two forms agree bit for bit wherever they hold the same entry (they share the accumulation code)."""
    torch = _t()
    ctx = gpu_ctx
    L = _layout(name, K)
    n_tiles, Rt, ranks, off = L["n_tiles"], L["Rt"], L["ranks"], L["col_off"]
    Rc = Rt + K
    G64, Ga = L["G64"], L["Ga"]
    # dense form
    ldg = Rc + 3
    G = torch.full((Rc, ldg), float("nan"), device=ctx.device)
    ctx.call("pmd_gram_u", P(L["Uw"]), L["dpad"], L["b1"], L["b2"], P(L["pix"]), P(L["pairs_dev"]), L["pairs"].shape[0],
             P(L["origins"]), P(L["col_off_dev"]), P(L["ranks_dev"]), n_tiles, Rt, P(L["basis"]), L["D"], K, P(G), ldg)
    ctx.sync()
    Gh = G.cpu().numpy()
    ok = _within_one_ulp(Gh[:, :Rc], G64, Ga)
    assert ok.all(), ("gram_u", np.argwhere(~ok)[:5], int((~ok).sum()))
    # block form
    ldgs = Rc + 5
    gblk, gbg, gstrip = _gram_blocks(ctx, L, ldgs)
    gblk, gbg, gstrip = gblk.cpu().numpy(), gbg.cpu().numpy(), gstrip.cpu().numpy()
    for p, (a, b) in enumerate(L["pairs"][:, :2]):
        ra, rb = int(ranks[a]), int(ranks[b])
        blk = gblk[p]
        assert np.all(blk[ra:, :] == 0) and np.all(blk[:, rb:] == 0), ("Gblk beyond the ranks", p)
        ref = G64[off[a]:off[a] + ra, off[b]:off[b] + rb]
        ok = _within_one_ulp(blk[:ra, :rb], ref, Ga[off[a]:off[a] + ra, off[b]:off[b] + rb])
        assert ok.all(), ("Gblk", p, a, b, np.argwhere(~ok)[:5])
    if K > 0:
        for kb in range((K + 63) // 64):
            kc = min(64, K - 64 * kb)
            for t in range(n_tiles):
                blk = gbg[kb * n_tiles + t]
                r = int(ranks[t])
                assert np.all(blk[r:, :] == 0) and np.all(blk[:, kc:] == 0), ("Gbg beyond the ranks", kb, t)
                sl = (slice(off[t], off[t] + r), slice(Rt + 64 * kb, Rt + 64 * kb + kc))
                assert _within_one_ulp(blk[:r, :kc], G64[sl], Ga[sl]).all(), ("Gbg", kb, t)
        ok = _within_one_ulp(gstrip[:K, :Rc], G64[Rt:, :], Ga[Rt:, :])
        assert ok.all(), ("Gstrip", np.argwhere(~ok)[:5])
        assert np.all(gstrip[:K, Rc:] == 0)   # (the strip is cleared over its leading dimension)
    # the dense and the block form are two stores of the same fp64 sums (same terms, same order): bit for bit
    for p, (a, b) in enumerate(L["pairs"][:, :2]):
        ra, rb = int(ranks[a]), int(ranks[b])
        assert np.array_equal(Gh[off[a]:off[a] + ra, off[b]:off[b] + rb], gblk[p][:ra, :rb]), ("G vs Gblk", p, a, b)
    for k in range(K):
        kb, kk = divmod(k, 64)
        for t in range(n_tiles):
            r = int(ranks[t])
            col = gbg[kb * n_tiles + t][:r, kk]
            assert np.array_equal(Gh[off[t]:off[t] + r, Rt + k], col), ("G vs Gbg", k, t)
            assert np.array_equal(gstrip[k, off[t]:off[t] + r], col), ("Gstrip vs Gbg", k, t)
    if K > 0:
        assert np.array_equal(Gh[Rt:, :Rc], gstrip[:K, :Rc]), "G[Rt:, :] vs Gstrip"
        assert np.array_equal(Gh[Rt:, Rt:Rc], gstrip[:K, Rt:Rc]), "G[Rt:, Rt:] vs the strip's background block"


def _apply(ctx, L, gb, M, ldm, ncols, GM, ldgm, a0=0):
    torch = _t()
    K, n_tiles, Rt = L["K"], L["n_tiles"], L["Rt"]
    nbr_ptr, nbr = L["nbr"]
    ctx.call("pmd_gram_apply", P(gb[0]), P(gb[1]), P(gb[2]), Rt + K, P(nbr_ptr[a0:]), P(nbr), P(L["col_off_dev"][a0:]),
             P(L["ranks_dev"][a0:]), n_tiles - a0, Rt, K, int(L["ranks"].max()), P(M), ldm, ncols, P(GM), ldgm)


@functools.lru_cache(maxsize=1)
def _apply_setup(name, cap):
    torch = _t()
    L = dict(_layout(name, 70, cap))
    nbr_ptr, nbr = grid.neighbour_lists(L["pairs"], L["ranks"], L["col_off"][:-1], L["n_tiles"], L["Rt"], L["K"])
    dev = torch.device("cuda", 0)
    L["nbr"] = (torch.from_numpy(nbr_ptr.astype(np.int32)).to(dev), torch.from_numpy(np.ascontiguousarray(nbr, dtype=np.int32)).to(dev))
    return L


@pytest.fixture(scope="module")
def plain_apply_ctx():
    """One context for all "plain" cases below, created under PMD_GRAM_APPLY_MFMA=0."""
    ctx = context_under({"PMD_GRAM_APPLY_MFMA": "0"})
    yield ctx
    ctx.close()


@pytest.mark.parametrize("ncols", [1, 3, 4, 255, 257, 1000])
@pytest.mark.parametrize("kernel", ["mfma", "plain"])
@pytest.mark.parametrize("layout", [("grid70x80", 16), ("grid70x80", 32), ("snapped73x82", 48), ("grid70x80", 64),
                                    ("virtual", 64)])
def test_gram_apply_matches_float64(gpu_ctx, plain_apply_ctx, layout, kernel, ncols):
    """pmd_gram_apply (GM = G M on the block-sparse G) against float64 G M with the same fp32 G: element-wise within
    n 2^-24 (|G| |M|), n the terms of the row (any summation order); both kernels, every max_rank bucket (tile ranks capped
    at 16 / 32 / 48 / 64: MFMA CT 1-4, plain 16 / 32 / 64); columns >= ncols of GM untouched; a call on a tile sub-range
    (the sharded driver's call) gives those tiles' rows bit for bit."""
    torch = _t()
    ctx = gpu_ctx if kernel == "mfma" else plain_apply_ctx
    name, cap = layout
    L = _apply_setup(name, cap)
    K, Rt = L["K"], L["Rt"]
    Rc = Rt + K
    gb = _gram_blocks(ctx, L)
    if kernel == "mfma":
        ldm = (ncols + 1 + 3) // 4 * 4           # ncols = ldm - 1 where ncols % 4 == 3 (the driver's "drop" shape)
        ldgm = ldm
        Mbuf = torch.empty((Rc * ldm,), device=ctx.device)
        GMbuf = torch.full((Rc * ldgm,), float("nan"), device=ctx.device)
        M, GM = Mbuf.view(Rc, ldm), GMbuf.view(Rc, ldgm)
    else:
        ldm = ncols + (1 if ncols % 2 == 0 else 2)    # odd
        ldgm = ldm + 2
        Mbuf = torch.empty((Rc * ldm + 1,), device=ctx.device)
        GMbuf = torch.full((Rc * ldgm + 1,), float("nan"), device=ctx.device)
        M, GM = Mbuf[1:].view(Rc, ldm), GMbuf[1:].view(Rc, ldgm)   # one float off 16-byte alignment
    g = torch.Generator(device=ctx.device).manual_seed(ncols * 7 + cap)
    M.copy_(torch.randn((Rc, ldm), device=ctx.device, generator=g))
    _apply(ctx, L, gb, M, ldm, ncols, GM, ldgm)
    ctx.sync()
    G32 = torch.from_numpy(L["G64"].astype(np.float32).astype(np.float64)).to(ctx.device)
    Mref = M[:, :ncols].double()
    ref = G32 @ Mref
    bound = (torch.from_numpy(L["Ga"]).to(ctx.device) > 0).sum(1, keepdim=True).double() * U32 * (G32.abs() @ Mref.abs())
    got = GM[:, :ncols].double()
    err = (got - ref).abs()
    assert torch.isfinite(got).all()
    bad = err > bound
    assert not bad.any(), (kernel, name, cap, ncols, int(bad.sum()), float((err / bound.clamp_min(1e-300)).max()))
    assert torch.isnan(GM[:, ncols:]).all(), "columns >= ncols were written"
    # the sharded driver's call: the tiles from a0 on
    a0 = L["n_tiles"] // 3
    GM2 = torch.full_like(GMbuf, float("nan"))
    GM2v = GM2.view(Rc, ldgm) if kernel == "mfma" else GM2[1:].view(Rc, ldgm)
    _apply(ctx, L, gb, M, ldm, ncols, GM2v, ldgm, a0=a0)
    ctx.sync()
    r0 = int(L["col_off"][a0])
    assert torch.equal(GM2v[r0:Rt, :ncols], GM[r0:Rt, :ncols]), "tile sub-range differs from the full call"
    assert torch.equal(GM2v[Rt:, :ncols], GM[Rt:, :ncols])
    assert torch.isnan(GM2v[:r0]).all(), "rows of tiles before the sub-range were written"


# ------------------------------------------------------------------------------------------------------------------
# M^T G M

def _mtgm(ctx, M, rows, m, ldm, GM, ldgm, C, ldc, ws=None):
    torch = _t()
    if ws is None:
        nb = ctx.lib.pmd_gram_mtgm_workspace_bytes(rows, m)
        ws = torch.empty(((nb + 3) // 4,), dtype=torch.float32, device=ctx.device)
    ctx.call("pmd_gram_mtgm", P(M), rows, m, ldm, P(GM), ldgm, P(C), ldc, P(ws), ws.numel() * 4)
    return ws


@pytest.mark.parametrize("m,rows", [(1, 131), (90, 217), (300, 637), (515, 1067), (1000, 20000)])
def test_gram_mtgm_structure_and_fp32_routes(gpu_ctx, m, rows):
    """pmd_gram_mtgm on padded operands (ldm, ldgm, ldc beyond m; rows not a multiple of 64): every row block's lower
    triangle and diagonal finite and within rows 2^-24 (|M|^T |GM|) of float64; entries right of each row block's triangle
    still NaN; the first m x pmd_gram_mtgm_ld(rows) floats of the workspace hold M^T bit for bit (the driver reuses them
    for M^T Z).  rows = 20 000 at m = 1000 takes the split-K product."""
    torch = _t()
    ctx = gpu_ctx
    ldm, ldgm, ldc = m + 3, m + 5, m + 2
    g = torch.Generator(device=ctx.device).manual_seed(m)
    M = torch.randn((rows, ldm), device=ctx.device, generator=g)
    GM = torch.randn((rows, ldgm), device=ctx.device, generator=g)
    GM[:, :m] += M[:, :m]
    Cg = torch.full((m, ldc), float("nan"), device=ctx.device)
    ws = _mtgm(ctx, M, rows, m, ldm, GM, ldgm, Cg, ldc)
    ctx.sync()
    C64 = _mtgm64(torch, M, GM, rows, m)
    Cabs = M[:, :m].double().abs().T @ GM[:, :m].double().abs()
    bs = _mtgm_block_size(m)
    for i0 in range(0, m, bs):
        i1 = min(m, i0 + bs)
        blk = Cg[i0:i1, :i1]
        low = torch.tril(torch.ones((i1 - i0, i1), dtype=torch.bool, device=ctx.device), diagonal=i0)
        assert torch.isfinite(blk[low]).all(), ("non-finite in the lower triangle", i0)
        err = (blk.double() - C64[i0:i1, :i1]).abs()[low]
        bound = rows * U32 * Cabs[i0:i1, :i1][low]
        assert (err <= bound).all(), (i0, float((err / bound).max()))
        assert torch.isnan(Cg[i0:i1, i1:]).all(), ("written right of the row block", i0)
    assert torch.isnan(Cg[:, m:]).all()
    ld = int(ctx.lib.pmd_gram_mtgm_ld(rows))
    Mt = ws[:m * ld].view(m, ld)[:, :rows]
    assert torch.equal(Mt, M[:, :m].T.contiguous()), "workspace does not start with M^T"


def _mtgm_errors(ctx, M, GM, rows, m, C64, bs):
    torch = _t()
    Cg = torch.full((m, m), float("nan"), device=ctx.device)
    prof = _profiled(ctx, lambda: _mtgm(ctx, M, rows, m, m, GM, m, Cg, m))
    errs = _block_errors(Cg, C64, m, bs)
    del Cg
    return errs, prof


def _mtgm_operands(torch, device, rows, m, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    M = torch.randn((rows, m), device=device, generator=g)
    GM = torch.randn((rows, m), device=device, generator=g).mul_(0.5).add_(M)
    return M, GM


def test_gram_mtgm_concatenated_route(gpu_ctx):
    """The concatenated fp16-piece route of pmd_gram_mtgm at its default gates: m = 4096 (row blocks of 1024: 256 output
    macro tiles), rows = 12 500 (above 100 GFLOP per row block; 13 accumulation chunks of 1024, the last one ragged).  The
    profile shows gemm_f16x2; every row block's error against float64 stays at the level of the fp32 route of a
    PMD_GEMM_SPLIT=0 context.  Measured on MI355X: 0.98-1.33e-7 per row block, against 2.2-3.3e-7 from the fp32 route
    (ratio <= 0.45); bounds 2e-7 and 0.75 x the fp32 route."""
    torch = _t()
    ctx = gpu_ctx
    m, rows = 4096, 12500
    M, GM = _mtgm_operands(torch, ctx.device, rows, m, 11)
    C64 = _mtgm64(torch, M, GM, rows, m)
    bs = _mtgm_block_size(m)
    errs, prof = _mtgm_errors(ctx, M, GM, rows, m, C64, bs)
    assert "gemm_f16x2" in prof, prof
    ref_ctx = _fresh_ctx(split=False)
    try:
        errs32, prof32 = _mtgm_errors(ref_ctx, M, GM, rows, m, C64, bs)
    finally:
        ref_ctx.close()
    assert "gemm_f16x2" not in prof32
    for e, e32 in zip(errs, errs32):
        assert e < 2e-7 and e < 0.75 * e32, (errs, errs32)


@pytest.mark.parametrize("m,rows", [(1000, 309827), (2000, 110576)])
def test_gram_mtgm_fallback_keeps_the_fp32_product(gpu_ctx, m, rows):
    """Where the concatenated route is gated off (fewer than 256 output macro tiles: the many-tile workloads of bench.py,
    1024x1024x1000_b16 and 1024x1024x2000_b32), every row block of pmd_gram_mtgm is the fp32 product: no fp16-piece product
    in the profile of the call (a two-piece product over the whole inner dimension is the arithmetic that breaks this
    product), and every row block's error against float64 at most 1.5 x that of a PMD_GEMM_SPLIT=0 context.  (Measured on
    MI355X with a two-piece product in the fallback: row block 512 of 1000 x 309 827 at 9.5e-7 against 2.2e-7 from the fp32
    product; at 2000 x 110 576 row blocks 512 / 1024 at 5.9e-7 / 6.1e-7 against 3.4e-7 / 5.2e-7.)"""
    torch = _t()
    ctx = gpu_ctx
    M, GM = _mtgm_operands(torch, ctx.device, rows, m, m)
    C64 = _mtgm64(torch, M, GM, rows, m)
    bs = _mtgm_block_size(m)
    errs, prof = _mtgm_errors(ctx, M, GM, rows, m, C64, bs)
    ref_ctx = _fresh_ctx(split=False)
    try:
        errs32, _ = _mtgm_errors(ref_ctx, M, GM, rows, m, C64, bs)
    finally:
        ref_ctx.close()
    for e, e32 in zip(errs, errs32):
        assert e <= 1.5 * e32, (errs, errs32)
    assert "gemm_f16x2" not in prof and "f16x2_split" not in prof, sorted(prof)


def test_gemm_mtz_many_tile_shape(gpu_ctx):
    """pmd_gemm as the driver calls it for M^T Z at the many-tile shape (1000 x 1000 x 309 827, M^T at leading dimension
    pmd_gram_mtgm_ld): error against float64 at most 1.5 x that of the split-K sgemm route (PMD_GEMM_SPLIT=0 context).
    Measured on MI355X: 1.56e-6 from the two-piece product over the whole inner dimension, 3.5e-6 from split-K sgemm."""
    torch = _t()
    ctx = gpu_ctx
    m, T, rows = 1000, 1000, 309827
    ld = int(ctx.lib.pmd_gram_mtgm_ld(rows))
    g = torch.Generator(device=ctx.device).manual_seed(4)
    Mt = torch.randn((m, ld), device=ctx.device, generator=g)
    Z = torch.randn((rows, T), device=ctx.device, generator=g).add_(0.3)
    ref = torch.zeros((m, T), dtype=torch.float64, device=ctx.device)
    for r0 in range(0, rows, 32768):
        r1 = min(rows, r0 + 32768)
        ref += Mt[:, r0:r1].double() @ Z[r0:r1].double()
    errs = []
    for split in (True, False):
        cx = ctx if split else _fresh_ctx(split=False)
        try:
            W1 = torch.empty((m, T), device=ctx.device)
            cx.call("pmd_gemm", 0, 0, m, T, rows, 1.0, P(Mt), ld, P(Z), T, 0.0, P(W1), T)
            cx.sync()
            errs.append(float(((W1.double() - ref).norm() / ref.norm()).item()))
        finally:
            if not split:
                cx.close()
    assert errs[0] <= 1.5 * errs[1], errs


# ------------------------------------------------------------------------------------------------------------------
# Cholesky step

def _spd(rng, m, kappa):
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    lam = np.logspace(0, -np.log10(kappa), m) if m > 1 else np.ones(1)
    return (Q * lam) @ Q.T


def _chol_call(ctx, C32, m, ldc, abs_last):
    torch = _t()
    buf = np.full((m, ldc), 7.0, dtype=np.float32)
    buf[:, :m] = C32
    Cd = torch.from_numpy(buf).to(ctx.device)
    ok = C.c_int(-1)
    ws = ctx.workspace(ctx.lib.pmd_chol_inverse_workspace_bytes(m))
    ctx.call("pmd_chol_inverse", P(Cd), m, ldc, abs_last, C.byref(ok), P(ws), ws.numel())
    ctx.sync()
    return ok.value, Cd.cpu().numpy()


def _et_ref(C64, abs_last):
    """float64 inverse Cholesky factor Et = L^{-1} (C = L L^T); abs_last: the last pivot through |Schur complement|."""
    m = C64.shape[0]
    L = np.zeros_like(C64)
    if abs_last:
        L11 = np.linalg.cholesky(C64[:m - 1, :m - 1]) if m > 1 else np.zeros((0, 0))
        y = np.linalg.solve(L11, C64[m - 1, :m - 1]) if m > 1 else np.zeros(0)
        L[:m - 1, :m - 1] = L11
        L[m - 1, :m - 1] = y
        L[m - 1, m - 1] = np.sqrt(abs(C64[m - 1, m - 1] - y @ y))
    else:
        L = np.linalg.cholesky(C64)
    return np.linalg.inv(L)


CHOL_ORDERS = [1, 2, 64, 512, 513, 640, 641, 1030]   # <= 512: the fp64 route; beyond: the library's fp32 chain (128-row blocks)


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("m", CHOL_ORDERS)
def test_chol_inverse_spd(gpu_ctx, m, pad):
    """pmd_chol_inverse on SPD C with a prescribed spectrum (kappa 1e2 and 1e6): ok = 1; Et lower triangular with exact zeros
    above the diagonal, padding columns untouched; Et against the float64 inverse Cholesky factor of the same fp32 C, within
    2 2^-24 |Et| plus the fp64 factorisation's own term on the fp64 route and 0.25 kappa 2^-24 max|Et| on the fp32 chain
    (measured on MI355X: 0.03-0.10 kappa 2^-24 over these orders and both kappa)."""
    rng = np.random.default_rng(m + pad)
    ldc = m + pad
    for kappa in (1e2, 1e6):
        C32 = _spd(rng, m, kappa).astype(np.float32)
        C32 = ((C32 + C32.T) / 2).astype(np.float32)
        ok, out = _chol_call(gpu_ctx, C32, m, ldc, 0)
        assert ok == 1, (m, kappa)
        E = out[:, :m].astype(np.float64)
        assert np.all(out[:, m:] == 7.0), "padding columns written"
        assert np.all(np.triu(E, 1) == 0.0)
        ref = _et_ref(C32.astype(np.float64), 0)
        scale = np.abs(ref).max()
        err = np.abs(E - ref)
        if m <= 512:
            bound = 2 * U32 * np.abs(ref) + kappa * m * 2.0 ** -50 * scale
            assert np.all(err <= bound), (m, kappa, float((err / bound).max()))
        else:
            rel = float(err.max() / scale)
            assert rel <= 0.25 * kappa * U32, (m, kappa, rel)


@pytest.mark.parametrize("m", [2, 64, 512, 513, 640, 641, 1030])
def test_chol_inverse_abs_last_pivot(gpu_ctx, m):
    """abs_last_pivot: leading block SPD, last Schur complement negative but resolved (-delta, delta = 1e-3 of the mean
    diagonal).  abs_last_pivot = 1: ok = 1 and Et is the float64 inverse of the factor whose last pivot is sqrt(delta);
    abs_last_pivot = 0: ok = 0.  An indefinite leading block: ok = 0 with either flag and no error; on the fp64 route C is
    left untouched (its documented contract)."""
    rng = np.random.default_rng(1000 + m)
    A = _spd(rng, m - 1, 1e2)
    md = np.mean(np.diag(A))
    delta = 1e-3 * md
    # coupling b = A x with x^T A x = 1e-2 of the mean diagonal: C_mm = x^T A x - delta cancels one decimal digit only (a
    # larger coupling makes the pivot unresolvable in fp32, whatever the factorisation)
    x = rng.standard_normal(m - 1)
    x *= np.sqrt(1e-2 * md / (x @ A @ x))
    b = A @ x
    C64 = np.zeros((m, m))
    C64[:m - 1, :m - 1] = A
    C64[m - 1, :m - 1] = C64[:m - 1, m - 1] = b
    C64[m - 1, m - 1] = x @ A @ x - delta
    C32 = C64.astype(np.float32)
    ok, out = _chol_call(gpu_ctx, C32, m, m + 1, 1)
    assert ok == 1, m
    ref = _et_ref(C32.astype(np.float64), 1)
    E = out[:, :m].astype(np.float64)
    assert np.all(np.triu(E, 1) == 0.0)
    # the leading rows are the factor of the SPD block (kappa 1e2); the last row carries the resolved pivot
    lead = float(np.abs(E[:m - 1] - ref[:m - 1]).max() / np.abs(ref[:m - 1]).max())
    last = float(np.abs(E[m - 1] - ref[m - 1]).max() / np.abs(ref[m - 1]).max())
    # measured on MI355X: lead / last 4.7e-8 / 2.3e-8 on the fp64 route, 8.6e-7 / 9.8e-7 on the fp32 chain
    assert lead <= (2 * U32 if m <= 512 else 0.5 * 1e2 * U32), (m, lead)
    assert last <= (2e-7 if m <= 512 else 1e-5), (m, last)
    ok0, _ = _chol_call(gpu_ctx, C32, m, m + 1, 0)
    assert ok0 == 0, m
    # indefinite leading block
    Q, _ = np.linalg.qr(rng.standard_normal((m - 1, m - 1)))
    lam = np.linspace(1.0, 0.1, m - 1)
    lam[(m - 1) // 2] = -0.5
    Cind = np.zeros((m, m))
    Cind[:m - 1, :m - 1] = (Q * lam) @ Q.T
    Cind[m - 1, m - 1] = 1.0
    Cind = Cind.astype(np.float32)
    for flag in (0, 1):
        ok_i, out_i = _chol_call(gpu_ctx, Cind, m, m + 1, flag)
        assert ok_i == 0, (m, flag)
        if m <= 512:
            assert np.array_equal(out_i[:, :m], Cind), "the fp64 route changed C on failure"


def test_cholesky_chain_headline_structure(gpu_ctx):
    """The driver's exact sequence on the headline's structure: 130 x 130 field of view, 10 x 10 blocks, 625 tiles of rank
    20, K = 3 (m = 4096 frames, Rc = 12 503); `right` holds traces centred over the frames (the constant vector is null).
    Householder rotation of the null direction into the last column, pmd_gram_apply, pmd_gram_mtgm, pmd_chol_inverse
    (abs_last_pivot = 1): ok = 1, the leading (m - 1) block of Et C64 Et^T within a stated bound of I (C64 the float64
    M^T G M of the same fp32 inputs), the last pivot at rounding level."""
    import math

    torch = _t()
    ctx = gpu_ctx
    L = dict(_layout("headline", 3))
    K, Rt, n_tiles = L["K"], L["Rt"], L["n_tiles"]
    Rc, m = Rt + K, 4096
    assert n_tiles == 625 and Rt == 12500
    nbr_ptr, nbr = grid.neighbour_lists(L["pairs"], L["ranks"], L["col_off"][:-1], n_tiles, Rt, K)
    L["nbr"] = (_i32(ctx, nbr_ptr), _i32(ctx, nbr))
    gb = _gram_blocks(ctx, L)
    g = torch.Generator(device=ctx.device).manual_seed(21)
    right = torch.randn((Rc, m), device=ctx.device, generator=g)
    right -= right.mean(dim=1, keepdim=True)
    # decomposition.py: H e_m = 1 / sqrt(m)
    nhat = np.full(m, 1.0 / math.sqrt(m))
    hv = -nhat
    hv[-1] += 1.0
    hv /= np.linalg.norm(hv)
    hv_dev = torch.from_numpy(hv.astype(np.float32)).to(ctx.device)
    y = torch.empty((Rc, 1), device=ctx.device)
    ctx.call("pmd_gemm", 0, 0, Rc, 1, m, 1.0, P(right), m, P(hv_dev), 1, 0.0, P(y), 1)
    ctx.call("pmd_gemm", 0, 0, Rc, m, 1, -2.0, P(y), 1, P(hv_dev), m, 1.0, P(right), m)
    GM = torch.empty((Rc, m), device=ctx.device)
    _apply(ctx, L, gb, right, m, m, GM, m)
    Et = torch.empty((m, m), device=ctx.device)
    _mtgm(ctx, right, Rc, m, m, GM, m, Et, m)
    ctx.sync()
    # float64 M^T G M of the same fp32 inputs (G from its fp32 blocks, as the kernels read it)
    G32 = torch.from_numpy(L["G64"].astype(np.float32).astype(np.float64)).to(ctx.device)
    R64 = right.double()
    C64 = R64.T @ (G32 @ R64)
    del G32, R64
    diag_mean = float(C64.diagonal()[:m - 1].mean())
    ok = C.c_int(-1)
    ws = ctx.workspace(ctx.lib.pmd_chol_inverse_workspace_bytes(m))
    ctx.call("pmd_chol_inverse", P(Et), m, m, 1, C.byref(ok), P(ws), ws.numel())
    ctx.sync()
    assert ok.value == 1
    E = Et.double()
    S = E @ C64 @ E.T
    lead = float((S[:m - 1, :m - 1] - torch.eye(m - 1, dtype=torch.float64, device=ctx.device)).abs().max())
    pivot = 1.0 / float(E[m - 1, m - 1])
    # measured on MI355X: 1.6e-6 and a last pivot of 2.7e-13 of the mean diagonal
    assert lead < 1e-5, lead
    assert pivot ** 2 < 1e-10 * diag_mean, (pivot ** 2, diag_mean)


def test_orthogonalize_factored_indefinite(gpu_ctx):
    """pmd_orthogonalize_factored on an indefinite M^T G M (G M = G M with an indefinite G) with a cluster of eigenvalues at
    1e-5 of the largest: rows in |lambda|-descending order with Et C64 Et^T = diag(sign lambda); the default rule keeps
    every nonzero direction; with pmd_ctx_set_null_cutoff(1e-3) exactly the directions above the cutoff."""
    torch = _t()
    ctx = gpu_ctx
    m, Rc = 300, 900
    rng = np.random.default_rng(8)
    Q1, _ = np.linalg.qr(rng.standard_normal((Rc, m)))
    V, _ = np.linalg.qr(rng.standard_normal((m, m)))
    mag = np.logspace(0, -3.5, m)
    mag[-12:] = 1e-5 * (1 + 0.01 * np.arange(12))   # the cluster
    sign = np.where(rng.random(m) < 0.3, -1.0, 1.0)
    sign[0] = 1.0
    lam = mag * sign
    S = (V * lam) @ V.T
    M32 = Q1.astype(np.float32)
    GM32 = (Q1 @ S).astype(np.float32)       # G M with G = Q1 S Q1^T
    C64 = M32.astype(np.float64).T @ GM32.astype(np.float64)
    Md = torch.from_numpy(M32).to(ctx.device)
    GMd = torch.from_numpy(GM32).to(ctx.device)
    ws = ctx.workspace(ctx.lib.pmd_orthogonalize_factored_workspace_bytes(m))
    lam64 = np.linalg.eigvalsh(C64)
    order = np.argsort(-np.abs(lam64), kind="stable")
    try:
        for cutoff in (-1.0, 1e-3):
            ctx.call("pmd_ctx_set_null_cutoff", cutoff)
            Et = torch.zeros((m, m), device=ctx.device)
            rp = C.c_int(-1)
            ctx.call("pmd_orthogonalize_factored", P(Md), Rc, m, m, P(GMd), m, P(Et), m, C.byref(rp), P(ws), ws.numel())
            ctx.sync()
            expect = m if cutoff < 0 else int(np.sum(lam64 > cutoff * np.abs(lam64).max()))
            assert rp.value == expect, (cutoff, rp.value, expect)
            kept = order[:expect] if cutoff < 0 else order[np.isin(order, np.nonzero(lam64 > cutoff * np.abs(lam64).max())[0])]
            E = Et.cpu().numpy()[:expect].astype(np.float64)
            Sx = E @ C64 @ E.T
            target = np.diag(np.sign(lam64[kept]))
            dev_ = np.abs(Sx - target)
            # a direction of eigenvalue lambda carries an error of ~ |dC| / |lambda|: bound scaled by the pair's magnitudes
            scale = np.sqrt(np.abs(lam64[kept])[:, None] * np.abs(lam64[kept])[None, :])
            worst = float((dev_ * scale / np.abs(lam64).max()).max())
            # measured on MI355X: worst 1.1-1.4e-7, leading 50 x 50 within 1.8-3.5e-7 of diag(sign lambda)
            assert worst < 1e-6, (cutoff, worst)
            assert dev_[:50, :50].max() < 2e-6
    finally:
        ctx.call("pmd_ctx_set_null_cutoff", -1.0)


def _indefinite(rng, n):
    """Symmetric indefinite fp32 matrix with the spectrum of test_orthogonalize_factored_indefinite (3.5 decades, 30 %
    negative, a cluster of 12 at 1e-5 of the largest) and its float64 eigenvalues."""
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    mag = np.logspace(0, -3.5, n)
    mag[-12:] = 1e-5 * (1 + 0.01 * np.arange(12))
    sign = np.where(rng.random(n) < 0.3, -1.0, 1.0)
    sign[0] = 1.0
    S = (V * (mag * sign)) @ V.T
    G32 = ((S + S.T) / 2).astype(np.float32)
    G32 = np.ascontiguousarray(np.triu(G32) + np.triu(G32, 1).T)     # symmetric after rounding
    return G32, np.linalg.eigvalsh(G32.astype(np.float64))


def _orthogonalize(ctx, G, R, M, m, ldm, ldp):
    torch = _t()
    Pm = torch.full((R, ldp), 7.0, device=ctx.device)
    rp = C.c_int(-1)
    ws = ctx.workspace(ctx.lib.pmd_orthogonalize_workspace_bytes(R, m, 1 if M is not None else 0))
    ctx.call("pmd_orthogonalize", P(G.clone()), R, P(M), m, ldm, P(Pm), ldp, C.byref(rp), P(ws), ws.numel())
    ctx.sync()
    return Pm, rp.value


def test_orthogonalize_with_right_matrix_equals_factored_pair(gpu_ctx):
    """pmd_orthogonalize with a right matrix M is pmd_gemm (G M) + pmd_orthogonalize_factored (Et) + pmd_gemm (P = M Et^T):
    the same products through the same entry with the same leading dimensions and one shared eigen-solve epilogue, so the
    same R' and the same P bit for bit (checked on MI355X before the epilogue was shared: bit-identical there as well)."""
    torch = _t()
    ctx = gpu_ctx
    R, m = 200, 60
    rng = np.random.default_rng(31)
    G32, _ = _indefinite(rng, R)
    G = torch.from_numpy(G32).to(ctx.device)
    ldm, ldp = m + 3, m + 2
    M = torch.from_numpy(rng.standard_normal((R, ldm)).astype(np.float32)).to(ctx.device)
    P0, rp0 = _orthogonalize(ctx, G, R, M, m, ldm, ldp)
    GM = torch.empty((R, m), device=ctx.device)
    ctx.call("pmd_gemm", 0, 0, R, m, R, 1.0, P(G), R, P(M), ldm, 0.0, P(GM), m)
    Et = torch.zeros((m, m), device=ctx.device)
    rp = C.c_int(-1)
    ws = ctx.workspace(ctx.lib.pmd_orthogonalize_factored_workspace_bytes(m))
    ctx.call("pmd_orthogonalize_factored", P(M), R, m, ldm, P(GM), m, P(Et), m, C.byref(rp), P(ws), ws.numel())
    assert rp.value == rp0 and rp0 == m, (rp.value, rp0)
    P1 = torch.full((R, ldp), 7.0, device=ctx.device)
    ctx.call("pmd_gemm", 0, 1, R, rp0, m, 1.0, P(M), ldm, P(Et), m, 0.0, P(P1), ldp)
    ctx.sync()
    print("orthogonalize vs factored pair: max |dP| =", float((P0[:, :rp0] - P1[:, :rp0]).abs().max()),
          "max |P| =", float(P0[:, :rp0].abs().max()))
    assert torch.all(P0[:, rp0:] == 7.0), "padding of P_out written"
    assert torch.equal(P0, P1)


def test_orthogonalize_identity_right_matrix(gpu_ctx):
    """pmd_orthogonalize with M == NULL (m = R, the dense R <= frames route) on an indefinite G: columns of P in
    |lambda|-descending order with P^T G64 P = diag(sign lambda), the scaled measure and bound of
    test_orthogonalize_factored_indefinite; with pmd_ctx_set_null_cutoff(1e-3) exactly the directions above the cutoff."""
    torch = _t()
    ctx = gpu_ctx
    R = 150
    G32, lam64 = _indefinite(np.random.default_rng(32), R)
    G64 = G32.astype(np.float64)
    G = torch.from_numpy(G32).to(ctx.device)
    order = np.argsort(-np.abs(lam64), kind="stable")
    lmax = np.abs(lam64).max()
    try:
        for cutoff in (-1.0, 1e-3):
            ctx.call("pmd_ctx_set_null_cutoff", cutoff)
            Pm, rp = _orthogonalize(ctx, G, R, None, R, 0, R + 1)
            above = np.nonzero(lam64 > cutoff * lmax)[0]
            expect = R if cutoff < 0 else len(above)
            assert rp == expect, (cutoff, rp, expect)
            assert torch.all(Pm[:, R:] == 7.0), "padding of P_out written"
            kept = order[:expect] if cutoff < 0 else order[np.isin(order, above)]
            Pc = Pm.cpu().numpy()[:, :expect].astype(np.float64)
            dev_ = np.abs(Pc.T @ G64 @ Pc - np.diag(np.sign(lam64[kept])))
            scale = np.sqrt(np.abs(lam64[kept])[:, None] * np.abs(lam64[kept])[None, :])
            worst = float((dev_ * scale / lmax).max())
            print("orthogonalize, identity right matrix: cutoff", cutoff, "R'", rp, "worst", worst)
            # measured on MI355X: 9.2e-8 and 7.3e-8 (test_orthogonalize_factored_indefinite: 1.1-1.4e-7 at order 300)
            assert worst < 1e-6, (cutoff, worst)
    finally:
        ctx.call("pmd_ctx_set_null_cutoff", -1.0)


# ------------------------------------------------------------------------------------------------------------------
# projected SVD

def _factored(ctx, M, Rc, m, Et, rp, Z, T, et_lower=0, W1_in=None, R_out=True, X1=None, ldr=None, ldvt=None):
    torch = _t()
    ldr = rp if ldr is None else ldr
    ldvt = T if ldvt is None else ldvt
    R = torch.full((Rc, ldr), 7.0, device=ctx.device) if R_out else None
    s = torch.empty(rp, device=ctx.device)
    Vt = torch.full((rp, ldvt), 7.0, device=ctx.device)
    ws = ctx.workspace(ctx.lib.pmd_projected_svd_factored_workspace_bytes(Rc, m, rp, T))
    ctx.call("pmd_projected_svd_factored", P(M), Rc, m, m, P(Et), rp, m, P(Z), T, T, P(R), ldr, P(s), P(Vt), ldvt, P(None), 0,
             P(X1), P(W1_in), et_lower, P(ws), ws.numel())
    ctx.sync()
    return R, s, Vt


def _split(ctx, Et, rp, m, W1, T, parts, et_lower=0):
    """pmd_psvd_vp_gram over column parts, C summed as the all-reduce does, pmd_psvd_finish per part."""
    torch = _t()
    ldc = (rp + 3) // 4 * 4
    Csum = torch.zeros((rp, ldc), device=ctx.device)
    vps = []
    for c0, c1 in zip(parts[:-1], parts[1:]):
        nc = c1 - c0
        Vp = torch.empty((rp, nc), device=ctx.device)
        Cp = torch.zeros((rp, ldc), device=ctx.device)
        ctx.call("pmd_psvd_vp_gram", P(Et), rp, m, m, P(W1[:, c0:]), nc, T, et_lower, P(Vp), nc, P(Cp), ldc)
        ctx.sync()
        Csum += Cp      # (one part: 0 + x = x, bit for bit)
        vps.append(Vp)
    s = torch.empty(rp, device=ctx.device)
    W = torch.empty((rp, rp), device=ctx.device)
    Vts = []
    ws = ctx.workspace(ctx.lib.pmd_psvd_finish_workspace_bytes(rp))
    for (c0, c1), Vp in zip(zip(parts[:-1], parts[1:]), vps):
        Cw = Csum.clone()
        Vt = torch.empty((rp, c1 - c0), device=ctx.device)
        ctx.call("pmd_psvd_finish", P(Cw), ldc, rp, P(Vp), c1 - c0, c1 - c0, P(W), rp, P(s), P(Vt), c1 - c0, P(ws), ws.numel())
        ctx.sync()
        Vts.append(Vt)
    return s, W, torch.cat(Vts, dim=1)


def test_projected_svd_whole_and_split(gpu_ctx):
    """pmd_psvd_vp_gram + pmd_psvd_finish with nc = T reproduce pmd_projected_svd_factored's s and Vt bit for bit (the header's
    claim) and R formed from their W matches R_out; 2 and 3 ragged column parts agree to fp32 rounding; s and separated Vt
    rows against the float64 SVD of Et (M^T Z); et_lower = 1 (strmm) agrees with et_lower = 0; W1_in agrees with W1 formed
    inside; R_out = NULL + X1_out + pmd_gemm gives R_out; padding of ldvt / ldr untouched; two calls bit-identical."""
    torch = _t()
    ctx = gpu_ctx
    Rc, m, T = 900, 300, 700
    rp = m
    g = torch.Generator(device=ctx.device).manual_seed(17)
    M = torch.randn((Rc, m), device=ctx.device, generator=g)
    Et = torch.tril(torch.randn((m, m), device=ctx.device, generator=g) * 0.05 + torch.eye(m, device=ctx.device))
    Z = torch.randn((Rc, T), device=ctx.device, generator=g) * torch.logspace(0, -2, T, device=ctx.device)[None, :]
    R0, s0, Vt0 = _factored(ctx, M, Rc, m, Et, rp, Z, T, ldr=rp + 5, ldvt=T + 3)
    assert torch.all(R0[:, rp:] == 7.0) and torch.all(Vt0[:, T:] == 7.0), "padding written"
    R0, Vt0 = R0[:, :rp].clone(), Vt0[:, :T].clone()
    R0b, s0b, Vt0b = _factored(ctx, M, Rc, m, Et, rp, Z, T)
    assert torch.equal(s0, s0b) and torch.equal(Vt0, Vt0b) and torch.equal(R0, R0b), "two calls differ"
    # W1 = M^T Z as the factored call forms it (explicit transposed copy at ld round_up(Rc, 64), plain product)
    ldt = (Rc + 63) // 64 * 64
    Mt = torch.zeros((m, ldt), device=ctx.device)
    ctx.call("pmd_transpose", P(M), m, Rc, m, P(Mt), ldt)
    W1 = torch.empty((m, T), device=ctx.device)
    ctx.call("pmd_gemm", 0, 0, m, T, Rc, 1.0, P(Mt), ldt, P(Z), T, 0.0, P(W1), T)
    ctx.sync()
    s1, W, Vt1 = _split(ctx, Et, rp, m, W1, T, [0, T])
    assert torch.equal(s1, s0), float((s1 - s0).abs().max())
    assert torch.equal(Vt1, Vt0), float((Vt1 - Vt0).abs().max())
    s1b, Wb, Vt1b = _split(ctx, Et, rp, m, W1, T, [0, T])
    assert torch.equal(s1, s1b) and torch.equal(W, Wb) and torch.equal(Vt1, Vt1b), "two split calls differ"
    # R from the split route's W: X1 = Et^T W, R = M X1
    X1 = torch.empty((m, rp), device=ctx.device)
    ctx.call("pmd_gemm", 1, 0, m, rp, rp, 1.0, P(Et), m, P(W), rp, 0.0, P(X1), rp)
    R1 = torch.empty((Rc, rp), device=ctx.device)
    ctx.call("pmd_gemm", 0, 0, Rc, rp, m, 1.0, P(M), m, P(X1), rp, 0.0, P(R1), rp)
    ctx.sync()
    rscale = float(R0.abs().max())
    assert float((R1 - R0).abs().max()) < 1e-5 * rscale
    # ragged column parts
    sep = torch.ones(rp, dtype=torch.bool, device=ctx.device)
    lam0 = s0.double() ** 2
    gaps = (lam0[:-1] - lam0[1:]) / lam0[0]
    sep[:-1] &= gaps > 1e-3
    sep[1:] &= gaps > 1e-3
    for parts in ([0, 351, T], [0, 233, 467, T]):
        s2, _, Vt2 = _split(ctx, Et, rp, m, W1, T, parts)
        assert float((s2 - s0).abs().max()) < 1e-5 * float(s0[0]), parts
        sg = torch.sign((Vt2 * Vt0).sum(1, keepdim=True))
        assert float((Vt2 * sg - Vt0)[sep].abs().max()) < 1e-3, parts
    # against float64
    V64 = Et.double() @ (M.double().T @ Z.double())
    _, s64, Vt64 = torch.linalg.svd(V64, full_matrices=False)
    srel = float(((s0.double() - s64).abs() / s64[0]).max())
    sg = torch.sign((Vt0.double() * Vt64).sum(1, keepdim=True))
    vdev = float((Vt0.double() * sg - Vt64)[sep].abs().max())
    # measured on MI355X: s within 1.2e-6 of s_0, the 94 separated rows of Vt within 2.5e-6
    assert srel < 5e-6, srel
    assert vdev < 1e-5, vdev
    # strmm route, W1 supplied, R left to the caller
    Rl, sl, Vtl = _factored(ctx, M, Rc, m, Et, rp, Z, T, et_lower=1)
    assert float((sl - s0).abs().max()) < 1e-5 * float(s0[0])
    sg = torch.sign((Vtl * Vt0).sum(1, keepdim=True))
    assert float((Vtl * sg - Vt0)[sep].abs().max()) < 1e-3
    Rw, sw, Vtw = _factored(ctx, M, Rc, m, Et, rp, Z, T, W1_in=W1)
    assert torch.equal(sw, s0) and torch.equal(Vtw, Vt0) and torch.equal(Rw, R0), "W1_in differs from W1 formed inside"
    X1o = torch.empty((m, rp), device=ctx.device)
    _, sx, _ = _factored(ctx, M, Rc, m, Et, rp, Z, T, R_out=False, X1=X1o)
    Rx = torch.empty((Rc, rp), device=ctx.device)
    ctx.call("pmd_gemm", 0, 0, Rc, rp, m, 1.0, P(M), m, P(X1o), rp, 0.0, P(Rx), rp)
    ctx.sync()
    assert torch.equal(sx, s0) and torch.equal(Rx, R0), "R_out = NULL + X1_out + pmd_gemm differs from R_out"


def test_projected_svd_more_rows_than_columns_with_projection(gpu_ctx):
    """pmd_projected_svd with n1 > n2 and a projection P (rows_p x n1): eigenvectors of V^T V give Vt, left = V W / s and
    R_out = P left.  s and the separated rows of Vt against the float64 SVD of V, R_out against P64 left64 up to the same
    signs; V is left as it was; padding of ldr / ldvt untouched; two calls bit-identical."""
    torch = _t()
    ctx = gpu_ctx
    rows_p, n1, n2 = 50, 300, 120
    nk = n2
    ldp, ldv, ldr, ldvt = n1 + 2, n2 + 1, nk + 5, n2 + 3
    g = torch.Generator(device=ctx.device).manual_seed(23)
    Pm = torch.randn((rows_p, ldp), device=ctx.device, generator=g)
    V = torch.randn((n1, ldv), device=ctx.device, generator=g) * torch.logspace(0, -2, ldv, device=ctx.device)[None, :]
    V0 = V.clone()

    def run():
        R = torch.full((rows_p, ldr), 7.0, device=ctx.device)
        s = torch.empty(nk, device=ctx.device)
        Vt = torch.full((nk, ldvt), 7.0, device=ctx.device)
        ws = ctx.workspace(ctx.lib.pmd_projected_svd_workspace_bytes(rows_p, n1, n2))
        ctx.call("pmd_projected_svd", P(Pm), rows_p, ldp, P(V), n1, n2, ldv, P(R), ldr, P(s), P(Vt), ldvt, P(ws), ws.numel())
        ctx.sync()
        return R, s, Vt

    R0, s0, Vt0 = run()
    assert torch.equal(V, V0), "V was written"
    assert torch.all(R0[:, nk:] == 7.0) and torch.all(Vt0[:, n2:] == 7.0), "padding written"
    R1, s1, Vt1 = run()
    assert torch.equal(s0, s1) and torch.equal(Vt0, Vt1) and torch.equal(R0, R1), "two calls differ"
    R0, Vt0 = R0[:, :nk].double(), Vt0[:, :n2].double()
    left64, s64, Vt64 = torch.linalg.svd(V[:, :n2].double(), full_matrices=False)
    Rref = Pm[:, :n1].double() @ left64
    lam = s64 ** 2
    gaps = (lam[:-1] - lam[1:]) / lam[0]
    sep = torch.ones(nk, dtype=torch.bool, device=ctx.device)
    sep[:-1] &= gaps > 1e-3
    sep[1:] &= gaps > 1e-3
    srel = float(((s0.double() - s64).abs() / s64[0]).max())
    sg = torch.sign((Vt0 * Vt64).sum(1))
    vdev = float((Vt0 * sg[:, None] - Vt64)[sep].abs().max())
    rdev = float((R0 * sg[None, :] - Rref)[:, sep].abs().max() / Rref.abs().max())
    print("projected_svd n1 > n2: separated", int(sep.sum()), "srel", srel, "vdev", vdev, "rdev", rdev)
    assert int(sep.sum()) >= 10
    # measured on MI355X: s within 8.2e-8 of s_0, the 46 separated rows of Vt within 3.6e-6, their columns of R_out within
    # 4.3e-6 of max |R|; bounds four times that
    assert srel < 3.5e-7, srel
    assert vdev < 1.5e-5, vdev
    assert rdev < 2e-5, rdev
