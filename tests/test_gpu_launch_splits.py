"""
Every launcher that cuts a call into several launches, one item past its cut (GPU).  A launcher that walks its items in
chunks of 32768 or 65535 re-bases four to eight pointers per chunk by hand; a wrong one damages only the items behind the
first chunk, which no small test sees.

Periodic inputs: item t (tile, ROI, frame, row) carries pattern t % 7, expanded on the device with an index.  7 is coprime
to both chunk sizes, so the items on either side of a cut differ and a chunk that starts at the wrong item shows.  The
float64 reference is computed for the seven patterns only, and one comparison on the device (in slabs, to bound its
scratch) checks EVERY item against ref[t % 7], at the bound the entry's small test uses: bit equality for copies,
quantisation and integer sums, the derived or recorded bound elsewhere.  No tolerance is new.  Outputs lie inside a larger
allocation whose other rows and padding columns hold a sentinel that must survive.

Not here, because they are covered or cannot be:
  pmd_scale_rows                   test_gpu_prep_stage.test_scale_rows (D = 32768 + 70), every row.
  pmdk_tile_pool_bin               also small_la_ref.POOL_CASES "rows_two_chunks" / "tiles_two_chunks", one cut per call; here
                                   both cuts in one call.
  pmdk_tile_rowmix                 test_gpu_tile_contractions.test_tile_rowmix_many_tiles (32769 tiles, each its own matrix);
                                   here the two kernels that case does not select.
  pmdk_tile_gram, pmdk_tile_xbt    put the tiles on grid.x and issue one launch whatever their number; the launcher they
                                   feed inside the tile stage, pmd_launch_reduce_slices (float4 and scalar form), has no
                                   entry of its own and cuts only inside pmd_tiles_decompose / pmd_tiles_residual.
  launch_gather_rows (global.hip)  cuts at 32768 rows of an eigen-solve of that order: 8.6 GB for the matrix alone and
                                   hours of solve; not covered by any test.
"""
import numpy as np
import pytest

from oracle import philox
from tests import prep_ref, register_ref, small_la_ref
from tests.device_util import ELEM, PRE64, P, _t, dev, kept, prefilled

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
U64 = 2.0 ** -53
PERIOD = 7
CUT_TILES = 32768
CUT_ROWS = 65535
N_TILES = CUT_TILES + 3
N_ROWS = CUT_ROWS + 3
GUARD = 2                      # sentinel items in front of and behind every output
assert CUT_TILES % PERIOD and CUT_ROWS % PERIOD


def pattern_of(ctx, n):
    torch = _t()
    return torch.arange(n, device=ctx.device) % PERIOD


def expand(ctx, pat, n):
    """pat (7, ...) numpy -> (n, ...) on the device, item t = pat[t % 7]"""
    return dev(ctx, pat)[pattern_of(ctx, n)]


def slabs(n, item=1):
    """[a, b) ranges of the n items with about four million entries each (item: entries per item)"""
    step = max(1, (1 << 22) // max(1, int(item)))
    return [(a, min(n, a + step)) for a in range(0, n, step)]


def entries(t):
    return t[0].numel() if t.shape[0] else 1


def first_bad(bad):
    return _t().nonzero(bad)[:4].tolist()


def check_bits(ctx, got, want7, what):
    """got (n, ...) holds want7[t % 7] in item t, bit for bit (want7: numpy, the dtype of got)"""
    torch = _t()
    n = got.shape[0]
    assert tuple(got.shape[1:]) == tuple(want7.shape[1:]), (what, got.shape, want7.shape)
    view = {4: torch.int32, 8: torch.int64, 2: torch.int16}[got.element_size()]
    w = dev(ctx, want7).view(view)
    idx = pattern_of(ctx, n)
    for a, b in slabs(n, entries(got)):
        bad = got[a:b].contiguous().view(view) != w[idx[a:b]]
        assert not bool(bad.any().item()), (what, "items from", a, first_bad(bad))


def check_bound(ctx, got, ref7, bound7, what):
    """|got[t] - ref7[t % 7]| <= bound7[t % 7] in every entry of every item; a NaN where the reference has none fails"""
    n = got.shape[0]
    assert tuple(got.shape[1:]) == tuple(ref7.shape[1:]) == tuple(bound7.shape[1:]), (what, got.shape, ref7.shape)
    r, bnd = dev(ctx, ref7, np.float64), dev(ctx, bound7, np.float64)
    idx = pattern_of(ctx, n)
    worst = 0.0
    for a, b in slabs(n, entries(got)):
        err = (got[a:b].double() - r[idx[a:b]]).abs()
        lim = bnd[idx[a:b]]
        bad = ~(err <= lim)
        assert not bool(bad.any().item()), (what, "items from", a, first_bad(bad))
        pos = lim > 0
        if bool(pos.any().item()):
            worst = max(worst, float((err[pos] / lim[pos]).max().item()))
    print(f"\n{what}: largest error / bound over {n} items = {worst:.3g}")


# ---------------------------------------------------------------------------------------------- pmd_gather_frames
@pytest.mark.parametrize("D", [5, 300])
@pytest.mark.parametrize("src", ["uint16", "float32"])
def test_gather_frames(gpu_ctx, src, D):
    """65538 frames (two launches of the 65535-row grid), the source rows of the second launch with their own part of both
    index lists.  dst_rows is a permutation of the odd rows of dst; the even rows, the gaps, keep their fill, like the rows
    in front of and behind the array.  A copy: bit for bit."""
    torch, ctx = _t(), gpu_ctx
    n = N_ROWS
    rng = np.random.default_rng(D)
    n_src = 11                                                     # coprime to 7 and to the cut
    if src == "float32":
        frames, fill = rng.standard_normal((n_src, D)).astype(np.float32), np.float32(-7777.0)
        movie = dev(ctx, frames)
    else:
        frames, fill = rng.integers(0, 65535, (n_src, D)).astype(np.uint16), np.uint16(65535)
        movie = dev(ctx, frames.view(np.int16))
    g = torch.Generator(device=ctx.device).manual_seed(D)
    src_rows = ((torch.arange(n, device=ctx.device) * 3 + 2) % n_src).to(torch.int32)
    dst_rows = (2 * torch.randperm(n, device=ctx.device, generator=g) + 1).to(torch.int32)
    whole = torch.full((GUARD + 2 * n + GUARD, D), float(fill) if src == "float32" else int(np.int16(-1)), dtype=movie.dtype,
                       device=ctx.device)
    dst = whole[GUARD:GUARD + 2 * n]
    want = whole.clone()
    want[GUARD + dst_rows.long()] = movie[src_rows.long()]
    ctx.call("pmd_gather_frames", P(movie), ELEM[src], D, P(src_rows), P(dst_rows), n, P(dst))
    ctx.sync()
    same = torch.equal(whole.view(torch.int32), want.view(torch.int32)) if src == "float32" else torch.equal(whole, want)
    assert same, "a frame is not its source's copy, or a gap / a row around dst was written"


# ---------------------------------------------------------------------------------------------- pmd_bg_filter
@pytest.mark.parametrize("K", [2, 17, 65])
def test_bg_filter(gpu_ctx, K):
    """D = 65535 * 64 + 70 pixel rows: the second launch of every pass filters the last 70 rows, with its own rows of the
    input, of the output and of the basis.  K = 2 and 17 take the 16- and the 64-column kernel, K = 65 a second pass over
    column 64 alone that reads the first pass's output.  out = in - basis pj with a given pj (the basis is not orthonormal:
    the filter does not need it to be).  The bound of test_gpu_prep_stage.test_bg_filter, (K + 4) 2^-24 (|x| + |B| |pj|) per
    entry; columns [nf, ld) exact zeros; rows in front of and behind the output untouched; in place the same bits."""
    torch, ctx = _t(), gpu_ctx
    D, nf = CUT_ROWS * 64 + 70, 3
    ld = int(ctx.lib.pmd_time_ld(nf))
    ldp = ld + 96
    rng = np.random.default_rng(K)
    x7 = rng.standard_normal((PERIOD, nf)).astype(np.float32)
    b7 = rng.standard_normal((PERIOD, K)).astype(np.float32)
    pj = rng.standard_normal((K, nf)).astype(np.float32)
    ref7, bound7 = prep_ref.filter_ref(x7, b7, pj), prep_ref.filter_bound(x7, b7, pj, K)
    idx = pattern_of(ctx, D)
    whole_in = torch.full((GUARD + D + GUARD, ld), float("nan"), device=ctx.device)
    xs = whole_in[GUARD:GUARD + D]
    xs[:, :nf] = dev(ctx, x7)[idx]
    xs[:, nf:] = 0.0
    basis = dev(ctx, b7)[idx].contiguous()
    pjd = torch.zeros((K, ldp), device=ctx.device)
    pjd[:, :nf] = dev(ctx, pj)
    whole_out = prefilled(ctx, (GUARD + D + GUARD, ld))
    out = whole_out[GUARD:GUARD + D]
    ctx.call("pmd_bg_filter", P(xs), P(out), D, nf, ld, P(basis), K, P(pjd), ldp)
    ctx.sync()
    assert kept(whole_out[:GUARD]) and kept(whole_out[GUARD + D:]), "rows around the output written"
    assert bool((out[:, nf:].contiguous().view(torch.int32) == 0).all().item()), "columns [nf, ld) are not +0.0"
    check_bound(ctx, out[:, :nf], ref7, bound7, f"bg_filter K={K}")
    ctx.call("pmd_bg_filter", P(xs), P(xs), D, nf, ld, P(basis), K, P(pjd), ldp)
    ctx.sync()
    assert bool(torch.isnan(whole_in[:GUARD]).all().item()) and bool(torch.isnan(whole_in[GUARD + D:]).all().item())
    assert torch.equal(xs.view(torch.int32), out.view(torch.int32)), "in place gave other bits"


# ---------------------------------------------------------------------------------------------- pmd_roi_gather
def test_roi_gather_split_rois(gpu_ctx):
    """65538 split ROIs of two partial rows each: the reduction of the partial rows runs in two launches, the second with
    its own rows of the split table.  ROI k has the two segments of pattern k % 7 (1 to 64 pixels of a 64-pixel frame,
    weights 1 to 3); n = 300 frames are two blocks of the reduction along x.  Small integers, so every sum is exact in
    fp32 and the traces equal the float64 sums bit for bit in all three containers (as in
    test_gpu_traces.test_gather_boolean_masks_exact_for_every_container_and_length); columns [n, ldo) and the rows around
    the output keep their fill."""
    torch, ctx = _t(), gpu_ctx
    K, D, n, ldo = N_ROWS, 64, 300, 304
    rng = np.random.default_rng(3)
    lens = np.array([[1, 64], [64, 1], [7, 9], [63, 2], [33, 31], [5, 5], [64, 64]])          # pixels per segment
    starts = np.concatenate([[0], np.cumsum(lens.reshape(-1))])
    pix = np.concatenate([np.sort(rng.choice(D, p, replace=False)) for p in lens.reshape(-1)]).astype(np.int32)
    wt = rng.integers(1, 4, pix.size).astype(np.float32)
    Y = rng.integers(0, 1000, (n, D))
    w7 = np.zeros((PERIOD, D))
    for j in range(PERIOD):
        for s in range(2):
            q0, p = starts[2 * j + s], lens[j, s]
            np.add.at(w7[j], pix[q0:q0 + p], wt[q0:q0 + p])
    want7 = w7 @ Y.T.astype(np.float64)
    assert want7.max() < 2 ** 24
    k = torch.arange(K, device=ctx.device)
    pat = k % PERIOD
    st, ln = dev(ctx, starts[:-1].reshape(PERIOD, 2)), dev(ctx, lens)
    # segs[2 k + s] = {q0, p, partial row 2 k + s, to the workspace}; split[k] = {out row k, first partial row 2 k, 2 parts}
    segs = torch.stack([st[pat], ln[pat], torch.stack([2 * k, 2 * k + 1], 1), torch.ones((K, 2), dtype=torch.int64, device=ctx.device)],
                       dim=2).to(torch.int64).contiguous()
    split = torch.stack([k, 2 * k, torch.full_like(k, 2)], dim=1).to(torch.int64).contiguous()
    pixd, wtd = dev(ctx, pix), dev(ctx, wt)
    nbytes = int(ctx.lib.pmd_roi_gather_workspace_bytes(2 * K, n))
    assert nbytes == 4 * 2 * K * n
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=ctx.device)
    results = {}
    for src in ELEM:
        y = dev(ctx, Y.astype(np.float32) if src == "float32" else Y.astype(np.int16))
        whole = prefilled(ctx, (GUARD + K + GUARD, ldo))
        out = whole[GUARD:GUARD + K]
        ws.fill_(0xFF)
        ctx.call("pmd_roi_gather", P(y), ELEM[src], n, D, 2 * K, P(segs), P(pixd), P(wtd), 2 * K, K, P(split), P(out), ldo, P(ws),
                 nbytes)
        ctx.sync()
        assert kept(whole[:GUARD]) and kept(whole[GUARD + K:]) and kept(out[:, n:].contiguous()), (src, "fill around the traces")
        check_bits(ctx, out[:, :n], want7.astype(np.float32), f"roi_gather {src}")
        results[src] = out[:, :n].clone()
    assert torch.equal(results["uint16"], results["float32"]) and torch.equal(results["int16"], results["float32"])


# ---------------------------------------------------------------------------------------------- pmd_roi_combine
@pytest.mark.parametrize("outputs", ["den+res", "den", "res"])
@pytest.mark.parametrize("with_c", [True, False], ids=["C", "C-null"])
def test_roi_combine(gpu_ctx, with_c, outputs):
    """65538 traces of 300 frames, two launches, each with its own rows of C, offset, raw, den and res (leading dimensions
    all different).  d = C + offset rounded once, res = raw - d rounded once: the bits of the same two fp32 operations in
    NumPy.  An output that is not asked for and the padding of the ones that are keep their fill."""
    torch, ctx = _t(), gpu_ctx
    K, n = N_ROWS, 300
    ldc, ldr, ldd, lde = 301, 304, 303, 302
    rng = np.random.default_rng(5)
    c7 = (rng.standard_normal((PERIOD, n)) * 50).astype(np.float32)
    raw7 = (rng.standard_normal((PERIOD, n)) * 50 + 1000).astype(np.float32)
    off7 = (1000 + rng.standard_normal(PERIOD)).astype(np.float32)
    d7 = (c7 + off7[:, None]) if with_c else np.broadcast_to(off7[:, None], (PERIOD, n)).copy()
    r7 = raw7 - d7
    assert d7.dtype == np.float32 and r7.dtype == np.float32
    idx = pattern_of(ctx, K)
    C = torch.full((K, ldc), float("nan"), device=ctx.device)
    C[:, :n] = dev(ctx, c7)[idx]
    raw = torch.full((K, ldr), float("nan"), device=ctx.device)
    raw[:, :n] = dev(ctx, raw7)[idx]
    off = dev(ctx, off7)[idx].contiguous()
    den_w, res_w = prefilled(ctx, (GUARD + K + GUARD, ldd)), prefilled(ctx, (GUARD + K + GUARD, lde))
    den, res = den_w[GUARD:GUARD + K], res_w[GUARD:GUARD + K]
    want_den, want_res = "den" in outputs, "res" in outputs
    ctx.call("pmd_roi_combine", K, n, P(C if with_c else None), ldc, P(off), P(raw), ldr, P(den if want_den else None), ldd,
             P(res if want_res else None), lde)
    ctx.sync()
    for name, wanted, whole, arr, want7 in (("den", want_den, den_w, den, d7), ("res", want_res, res_w, res, r7)):
        if not wanted:
            assert kept(whole), (name, "written without being asked for")
            continue
        assert kept(whole[:GUARD]) and kept(whole[GUARD + K:]) and kept(arr[:, n:].contiguous()), (name, "fill around the output")
        check_bits(ctx, arr[:, :n], want7, f"roi_combine {name}")


# ---------------------------------------------------------------------------------------------- pmd_group_project
def test_group_project_wide_rows(gpu_ctx):
    """65538 wide rows, each the sum of two partial rows: group_reduce_kernel runs in two launches, the second with its own
    rows of the wide table.  The smallest groups the wide path takes: one row of U on 5 pixels per group (two groups per
    wide row, 131076 groups x 2 frame blocks of the n = 70 frames in the grid).  Wide row k has the two groups of pattern
    k % 7.  The bound of test_gpu_projection.test_group_project_against_fp64 per row: |Z - ref| / | |U|^T |Y_std| | <= 1e-6 in
    the 2-norm over the frames."""
    torch, ctx = _t(), gpu_ctx
    K, D, n, p, ldz = N_ROWS, 64, 70, 5, 72
    rng = np.random.default_rng(8)
    mean = (1000.0 + rng.uniform(-20, 20, D)).astype(np.float32)
    std = (10.0 * rng.uniform(0.8, 1.2, D)).astype(np.float32)
    Y = np.rint(mean[None, :] + std[None, :] * rng.standard_normal((n, D))).astype(np.float32)
    n_g = 2 * PERIOD                                              # distinct groups: (pattern, part)
    pix = np.stack([np.sort(rng.choice(D, p, replace=False)) for _ in range(n_g)]).astype(np.int32)          # (14, 5)
    A = np.zeros((n_g, 16, 64), dtype=np.float32)                 # A_g: 16 rows (one row tile) of p64 = 64 columns
    A[:, 0, :p] = rng.standard_normal((n_g, p)).astype(np.float32)
    ys = (Y.astype(np.float64) - mean) / std
    part = np.einsum("gq,fgq->gf", A[:, 0, :p].astype(np.float64), ys[:, pix])
    scale = np.einsum("gq,fgq->gf", np.abs(A[:, 0, :p]).astype(np.float64), np.abs(ys[:, pix]))
    ref7 = part.reshape(PERIOD, 2, n).sum(axis=1)
    scale7 = scale.reshape(PERIOD, 2, n).sum(axis=1)
    k = torch.arange(K, device=ctx.device)
    pat = k % PERIOD
    gid = torch.stack([2 * pat, 2 * pat + 1], dim=1)              # (K, 2) distinct group of (wide row, part)
    rows = torch.stack([2 * k, 2 * k + 1], dim=1)                 # its partial row of the workspace
    one = torch.ones_like(gid)
    # groups[g] = {pix_off, p, a_off, out_row, r, to_ws}; wide[k] = {z_row, ws_row0, parts, stride}
    groups = torch.stack([gid * p, one * p, gid * 16 * 64, rows, one, one], dim=2).to(torch.int64).contiguous()
    wide = torch.stack([k, 2 * k, torch.full_like(k, 2), torch.ones_like(k)], dim=1).to(torch.int64).contiguous()
    nbytes = int(ctx.lib.pmd_group_project_workspace_bytes(2 * K, n))
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=ctx.device)
    whole = prefilled(ctx, (GUARD + K + GUARD, ldz))
    Z = whole[GUARD:GUARD + K]
    yd, md, sd, pd, ad = dev(ctx, Y), dev(ctx, mean), dev(ctx, std), dev(ctx, pix), dev(ctx, A)
    ctx.call("pmd_group_project", P(yd), 0, n, D, P(md), P(sd), 2 * K, P(groups), P(pd), P(ad), 2 * K, K, P(wide), P(Z), ldz,
             P(ws), nbytes)
    ctx.sync()
    assert kept(whole[:GUARD]) and kept(whole[GUARD + K:]) and kept(Z[:, n:].contiguous()), "fill around Z"
    got = Z[:, :n].double()
    assert bool(torch.isfinite(got).all().item())
    err = torch.linalg.norm(got - dev(ctx, ref7)[pat], dim=1) / torch.linalg.norm(dev(ctx, scale7)[pat], dim=1)
    print(f"\ngroup_project wide rows: max row err {float(err.max().item()):.2e}")
    bad = ~(err < 1e-6)
    assert not bool(bad.any().item()), first_bad(bad)


# ---------------------------------------------------------------------------------------------- pmd_rng_normal
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("index_step", [1, 3])
def test_rng_normal(gpu_ctx, index_step, transpose):
    """32771 arrays of 3 x 5 in one call: the second launch starts at array index0 + 32768 index_step and at its own batch
    of the output.  Every batch against the NumPy restatement of the generator, at the atol of
    test_gpu_kernels.test_rng_matches_numpy_restatement (3e-6: the Philox words are exact, libm's and the device's
    Box-Muller differ in the last place); the padding of every batch and the batches around the output keep their fill.
    No period here: every array has its own index, so each of the 32771 is its own pattern."""
    ctx = gpu_ctx
    seed, stream, index0, batch, rows, cols = 0x1234ABCD5678, 4, 7, N_TILES, 3, 5
    r_out, c_out = (cols, rows) if transpose else (rows, cols)
    ld, pad_rows = c_out + 3, r_out + 1
    whole = prefilled(ctx, (GUARD + batch + GUARD, pad_rows, ld))
    out = whole[GUARD:GUARD + batch]
    ctx.call("pmd_rng_normal", seed, stream, index0, index_step, batch, rows, cols, transpose, P(out), ld, pad_rows * ld)
    ctx.sync()
    assert kept(whole[:GUARD]) and kept(whole[GUARD + batch:]), "batches around the output written"
    assert kept(out[:, r_out:].contiguous()) and kept(out[:, :, c_out:].contiguous()), "padding of a batch written"
    ref = philox.normals_many(seed, stream, index0 + index_step * np.arange(batch), rows * cols).reshape(batch, rows, cols)
    if transpose:
        ref = ref.transpose(0, 2, 1)
    got = out[:, :r_out, :c_out].cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref)
    print(f"\nrng_normal step {index_step} transpose {transpose}: max |got - restatement| = {np.nanmax(err):.3g}")
    bad = ~(err <= 3e-6)
    assert not bad.any(), np.argwhere(bad)[:4].tolist()


# ---------------------------------------------------------------------------------------------- gram.hip, small_la.hip
RANKS7 = np.array([0, 64, 1, 33, 63, 17, 64])        # ranks / counts of the seven patterns: 0 and the maximum among them
assert (CUT_TILES % PERIOD, RANKS7.min(), RANKS7.max()) == (1, 0, 64)


def test_weight_tiles_every_tile(gpu_ctx):
    """pmd_weight_tiles over 32771 tiles of 16 x 16 pixels (dpad 256): the second launch with its own tiles of Ut, pix, ranks
    and Uw.  Every tile against float64 at test_gpu_assembly's bound, |got - ref| <= 4 2^-24 |ref|; rows at or beyond the
    rank exactly +0.0 although Ut holds NaN there; the tiles around Uw untouched."""
    torch, ctx = _t(), gpu_ctx
    d, n_pix = 256, 5000
    dpad = int(ctx.lib.pmd_tile_dpad(d))
    assert dpad == 256
    rng = np.random.default_rng(1)
    ut7 = np.full((PERIOD, 64, dpad), np.nan, dtype=np.float32)
    for j, rk in enumerate(RANKS7):
        ut7[j, :rk] = rng.standard_normal((rk, d)).astype(np.float32)
    pix7 = rng.integers(0, n_pix, (PERIOD, d)).astype(np.int32)
    w = rng.integers(1, 11, d).astype(np.float32)
    cumw = rng.integers(1, 40, n_pix).astype(np.float32)
    ref7 = np.zeros((PERIOD, 64, dpad))
    for j, rk in enumerate(RANKS7):
        ref7[j, :rk] = ut7[j, :rk].astype(np.float64) * w[None, :].astype(np.float64) / cumw[pix7[j]][None, :].astype(np.float64)
    zero7 = np.zeros((PERIOD, 64, dpad), dtype=bool)
    for j, rk in enumerate(RANKS7):
        zero7[j, rk:] = True
    ut, pix, ranks = expand(ctx, ut7, N_TILES), expand(ctx, pix7, N_TILES), expand(ctx, RANKS7.astype(np.int32), N_TILES)
    wd, cd = dev(ctx, w), dev(ctx, cumw)
    whole = prefilled(ctx, (GUARD + N_TILES + GUARD, 64, dpad))
    uw = whole[GUARD:GUARD + N_TILES]
    ctx.call("pmd_weight_tiles", P(ut), dpad, P(pix), d, P(wd), P(cd), P(ranks), P(uw), N_TILES)
    ctx.sync()
    assert kept(whole[:GUARD]) and kept(whole[GUARD + N_TILES:]), "tiles around Uw written"
    check_bound(ctx, uw, ref7, 4 * U32 * np.abs(ref7), "weight_tiles")
    z, idx = dev(ctx, zero7), pattern_of(ctx, N_TILES)
    for a, b in slabs(N_TILES, 64 * dpad):
        bits = uw[a:b].view(torch.int32)
        assert bool((bits[z[idx[a:b]]] == 0).all().item()), ("padding is not +0.0, tiles from", a)


def test_compact_rows_every_tile(gpu_ctx):
    """pmd_compact_rows over 32771 tiles, T = 64: the second launch with its own tiles of Out and its own part of col_off and
    ranks.  Z, pre-filled, holds Out's rows below the rank bit for bit at col_off, and its fill in the row between two
    tiles, in the columns [T, ldz) and around the array."""
    torch, ctx = _t(), gpu_ctx
    T, ldo, ldz = 64, 72, 68
    rng = np.random.default_rng(2)
    out7 = rng.standard_normal((PERIOD, 64, ldo)).astype(np.float32)
    out7[:, :, T:] = np.inf
    for j, rk in enumerate(RANKS7):
        out7[j, rk:] = np.inf
    out = expand(ctx, out7, N_TILES)
    ranks = expand(ctx, RANKS7.astype(np.int32), N_TILES)
    step = ranks.long() + 1                                        # one row of Z between the tiles, one in front
    off = torch.cumsum(step, 0) - step + 1
    rows = int(step.sum().item()) + 1
    whole = prefilled(ctx, (GUARD + rows + GUARD, ldz))
    z = whole[GUARD:GUARD + rows]
    want = whole.clone()
    tile = torch.repeat_interleave(torch.arange(N_TILES, device=ctx.device), ranks.long())
    comp = torch.arange(tile.numel(), device=ctx.device) - (torch.cumsum(ranks.long(), 0) - ranks.long())[tile]
    want[GUARD + off[tile] + comp, :T] = out[tile, comp, :T]
    off32 = off.to(torch.int32)
    ctx.call("pmd_compact_rows", P(out), ldo, P(off32), P(ranks), T, P(z), ldz, N_TILES)
    ctx.sync()
    assert int(tile.numel()) == int(ranks.sum().item()) and int(tile[-1].item()) == N_TILES - 1
    assert torch.equal(whole.view(torch.int32), want.view(torch.int32))


def test_tiles_truncate_every_tile(gpu_ctx):
    """pmd_tiles_truncate over 32771 tiles of 64 rows at leading dimension 256: in every tile the rows below the count keep
    their bits (NaN among them) and the rows from it on are exactly +0.0; the tiles around U untouched."""
    ctx = gpu_ctx
    ld = 256
    rng = np.random.default_rng(3)
    u7 = rng.standard_normal((PERIOD, 64, ld)).astype(np.float32)
    u7[:, 40:, 3] = np.nan
    want7 = u7.copy()
    for j, k in enumerate(RANKS7):
        want7[j, k:] = 0.0
    whole = prefilled(ctx, (GUARD + N_TILES + GUARD, 64, ld))
    u = whole[GUARD:GUARD + N_TILES]
    u.copy_(expand(ctx, u7, N_TILES))
    counts = expand(ctx, RANKS7.astype(np.int32), N_TILES)
    ctx.call("pmd_tiles_truncate", P(u), ld, P(counts), N_TILES, 64)
    ctx.sync()
    assert kept(whole[:GUARD]) and kept(whole[GUARD + N_TILES:]), "tiles around U written"
    check_bits(ctx, u, want7, "tiles_truncate")


@pytest.mark.parametrize("which", ["both", "spatial", "temporal"])
def test_roughness(gpu_ctx, which):
    """pmdk_roughness over 32771 tiles of 7 x 9 pixels, 9 components, T = 256: each statistic's second launch with its own
    tiles of Ut, V and stats.  Every tile within the running bound of small_la_ref.spatial_stat / temporal_stat (the bound
    of test_gpu_tile_small_la.test_roughness), NaN exactly on the all-zero rows; rows from r on, the statistic whose input
    is NULL and the tiles around stats keep their fill."""
    torch, ctx = _t(), gpu_ctx
    case = small_la_ref.RoughCase(7, 9, 256, 9)
    b1, b2, T, r = case
    d = b1 * b2
    U6, V6 = small_la_ref.rough_inputs(case)
    U7, V7 = np.concatenate([U6, U6[:1, ::-1]]), np.concatenate([V6, V6[1:2, ::-1]])      # a seventh pattern: rows reversed
    ref7, bound7 = small_la_ref.rough_reference(case, U7, V7)
    assert np.isnan(ref7).any() and not np.isnan(ref7).all()
    u_ld, v_ld = small_la_ref.rough_u_ld(d), small_la_ref.rough_v_ld(T)
    hu = np.full((PERIOD, 64, u_ld), np.nan, dtype=np.float32)
    hv = np.full((PERIOD, 64, v_ld), np.nan, dtype=np.float32)
    hu[:, :r, :d], hv[:, :r, :T] = U7, V7
    u_d, v_d = expand(ctx, hu, N_TILES), expand(ctx, hv, N_TILES)
    whole = prefilled(ctx, (GUARD + N_TILES + GUARD, 64, 2))
    stats = whole[GUARD:GUARD + N_TILES]
    ctx.call("pmdk_roughness", P(u_d if which != "temporal" else None), 64 * u_ld, u_ld, b1, b2,
             P(v_d if which != "spatial" else None), 64 * v_ld, v_ld, T, r, P(stats), N_TILES)
    ctx.sync()
    assert kept(whole[:GUARD]) and kept(whole[GUARD + N_TILES:]), "tiles around stats written"
    assert kept(stats[:, r:].contiguous()), "rows from r on written"
    idx = pattern_of(ctx, N_TILES)
    for k, name in enumerate(("spatial", "temporal")):
        g = stats[:, :r, k].contiguous()
        if which not in ("both", name):
            assert kept(g), (which, name, "written without its input")
            continue
        nan7 = np.isnan(ref7[:, :, k])
        assert torch.equal(torch.isnan(g), dev(ctx, nan7)[idx]), (which, name, "NaN exactly on the all-zero rows")
        live = np.where(nan7, 0.0, ref7[:, :, k])
        check_bound(ctx, torch.nan_to_num(g, nan=0.0), live, np.where(nan7, 0.0, bound7[:, :, k]), f"roughness {name} ({which})")


# ---------------------------------------------------------------------------------------------- pmdk_tile_pool_bin
def test_tile_pool_bin_rows_and_tiles_cut_in_one_call(gpu_ctx):
    """32768 + 70 pixel rows and 32768 + 3 tiles in the same call: the second chunk of bin_average and the second chunk of
    tile_pool (which reads rows of xbar that the first wrote in its own second chunk: the odd tiles take their pixels
    from the last rows).  Every row and every tile against float64 at small_la_ref.pool_bounds, as in
    test_gpu_tile_small_la.test_tile_pool_bin; all the fills kept."""
    ctx = gpu_ctx
    R = small_la_ref
    case = R.PoolCase("rows_and_tiles_two_chunks", (2, 2), 2, 2, 8, None, CUT_TILES + 70, N_TILES, "normal", 32)
    inp = R.pool_inputs(case)
    X, pix, pool_q, Pn, nbins, a = inp["X"], inp["pix"], inp["pool_q"], inp["P"], inp["nbins"], case.a
    n_rows, n_tiles, d = X.shape[0], pix.shape[0], pix.shape[1]
    assert pix[1::2].min() >= CUT_TILES and pix.max() < n_rows
    ldx, ld_ab = int(ctx.lib.pmd_time_ld(case.T)), int(ctx.lib.pmd_time_ld(nbins))
    tile_stride = Pn * ld_ab + case.extra
    hx = np.full((n_rows, ldx), np.nan, dtype=np.float32)
    hx[:, :a * nbins] = X[:, :a * nbins]
    x_d, pix_d, pq_d = dev(ctx, hx), dev(ctx, pix), dev(ctx, pool_q)
    xbar_d = prefilled(ctx, (GUARD + n_rows + GUARD, ld_ab))
    abar_d = prefilled(ctx, (GUARD + n_tiles + GUARD, tile_stride))
    ctx.call("pmdk_tile_pool_bin", P(x_d), ldx, n_rows, P(pix_d), n_tiles, d, P(pq_d), pool_q.shape[1], Pn, a, nbins,
             P(xbar_d[GUARD:]), P(abar_d[GUARD:]), ld_ab, tile_stride)
    ctx.sync()
    for whole, n in ((xbar_d, n_rows), (abar_d, n_tiles)):
        assert kept(whole[:GUARD]) and kept(whole[GUARD + n:]), "rows / tiles around an output written"
    assert kept(xbar_d[:, nbins:].contiguous()) and kept(abar_d[:, Pn * ld_ab:].contiguous())
    blocks = abar_d[GUARD:GUARD + n_tiles, :Pn * ld_ab].reshape(n_tiles, Pn, ld_ab)
    assert kept(blocks[:, :, nbins:].contiguous()), "columns of abar from nbins on written"
    rx, rxabs, ra, raabs, cnt = R.pool_reference(X, pix, pool_q, a, nbins)
    gx = xbar_d[GUARD:GUARD + n_rows, :nbins].cpu().numpy().astype(np.float64)
    ga = blocks[:, :, :nbins].cpu().numpy().astype(np.float64)
    bx, ba = R.pool_bounds(a, rxabs, raabs, cnt)
    ex, ea = np.abs(gx - rx), np.abs(ga - ra)
    assert np.all(ex <= bx), ("xbar", np.argwhere(~(ex <= bx))[:4].tolist())
    assert np.all(ea <= ba), ("abar", np.argwhere(~(ea <= ba))[:4].tolist())
    print(f"\npool_bin: xbar err / bound {(ex[bx > 0] / bx[bx > 0]).max():.3g}, abar {(ea[ba > 0] / ba[ba > 0]).max():.3g}")


# ---------------------------------------------------------------------------------------------- pmdk_tile_rowmix
@pytest.mark.parametrize("route,n_out,ld_in,ld_out,length", [("scalar<4>", 3, 8, 12, 6), ("mfma 16 positions", 37, 9, 11, 6)])
def test_tile_rowmix_other_kernels(gpu_ctx, route, n_out, ld_in, ld_out, length):
    """The 32768-tile loop of pmdk_tile_rowmix on the kernels that tile_gemm_ref.ROWMIX_MANY does not reach: n_out <= 4 (the
    scalar kernel) and rows that are not 16-byte aligned (the 16-position MFMA kernel).  Per-tile mixing matrices and
    inputs of pattern t % 7, 50 input rows.  The bound of test_gpu_tile_contractions: fp64 accumulation in any order,
    n_in 2^-53 (|N|^T |In|) in the any-order form of tile_gemm_ref, plus the rounding to fp32, 2^-24 |ref|.  Rows
    [n_out, 64) exact zeros up to len; positions from len on and the tiles around Out keep their fill."""
    from tests import tile_gemm_ref as G

    ctx = gpu_ctx
    n_in = 50
    kernel = G.route_of_rowmix(n_out, length, ld_in, ld_out, 64 * ld_in, 64 * ld_out, N_TILES)
    assert kernel == ("tile_rowmix_kernel<4>" if n_out <= 4 else "tile_rowmix_mfma_kernel"), kernel
    rng = np.random.default_rng(n_out)
    data7 = rng.standard_normal((PERIOD, n_in, length)).astype(np.float32)
    mats7 = rng.standard_normal((PERIOD, n_in, n_out))
    ref7, absref7 = G.ref_rowmix(mats7, data7, np.longdouble)
    bound7 = G.any_order_bound(n_in, G.U64, absref7) + G.U32 * np.abs(ref7)
    hin = np.full((PERIOD, 64, ld_in), np.nan, dtype=np.float32)
    hin[:, :n_in, :length] = data7
    hn = np.full((PERIOD, 64, 64), np.nan)
    hn[:, :n_in, :n_out] = mats7
    in_d, n_d = expand(ctx, hin, N_TILES), expand(ctx, hn, N_TILES)
    whole = prefilled(ctx, (GUARD + N_TILES + GUARD, 64, ld_out))
    out = whole[GUARD:GUARD + N_TILES]
    ctx.call("pmdk_tile_rowmix", P(in_d), 64 * ld_in, ld_in, P(n_d), 4096, n_in, n_out, P(out), 64 * ld_out, ld_out, length, N_TILES)
    ctx.sync()
    assert kept(whole[:GUARD]) and kept(whole[GUARD + N_TILES:]) and kept(out[:, :, length:].contiguous()), (route, "fill written")
    assert bool((out[:, n_out:, :length] == 0).all().item()), (route, "rows [n_out, 64) must be zero up to len")
    check_bound(ctx, out[:, :n_out, :length], np.asarray(ref7, dtype=np.float64), np.asarray(bound7, dtype=np.float64),
                f"tile_rowmix {route}")


# ---------------------------------------------------------------------------------------------- wide.hip
WIDE_RP = 128


def test_wide_gram(gpu_ctx):
    """pmdk_wide_gram at rp = 128 over 32771 tiles, one position per row (the shortest length), symmetric and cross form:
    the second launch with its own tiles of In, In2 and G.  A product of two fp32 values is exact in fp64, so with one
    position the bound of test_gpu_tile_kernels_wide.test_wide_gram, len 2^-53 (|In| |In2|^T), asks for the exact product,
    and it is asserted as such.  G of a tile is 128 KB: 4.3 GB for the array."""
    torch, ctx = _t(), gpu_ctx
    rp, length, ld = WIDE_RP, 1, 4
    rng = np.random.default_rng(11)
    a7 = np.full((PERIOD, rp, ld), np.nan, dtype=np.float32)
    b7 = np.full((PERIOD, rp, ld), np.nan, dtype=np.float32)
    a7[:, :, :length] = rng.standard_normal((PERIOD, rp, length)).astype(np.float32)
    b7[:, :, :length] = rng.standard_normal((PERIOD, rp, length)).astype(np.float32)
    ad, bd = expand(ctx, a7, N_TILES), expand(ctx, b7, N_TILES)
    a64, b64 = a7[:, :, :length].astype(np.float64), b7[:, :, :length].astype(np.float64)
    whole = prefilled(ctx, (GUARD + N_TILES + GUARD, 1, rp, rp), double=True)
    G = whole[GUARD:GUARD + N_TILES]
    for second, s64 in ((None, a64), (bd, b64)):
        whole.view(torch.int64).fill_(PRE64)
        ctx.call("pmdk_wide_gram", P(ad), rp * ld, ld, length, N_TILES, 1, rp, P(G), P(second))
        ctx.sync()
        assert kept(whole[:GUARD]) and kept(whole[GUARD + N_TILES:]), "tiles around G written"
        ref7 = np.einsum("nit,njt->nij", a64, s64)
        bound7 = length * U64 * np.einsum("nit,njt->nij", np.abs(a64), np.abs(s64))
        check_bound(ctx, G[:, 0], ref7, bound7, f"wide_gram cross={second is not None}")
        if length == 1:
            check_bits(ctx, G[:, 0], ref7, "wide_gram, exact product")


def test_wide_rowmix(gpu_ctx):
    """pmdk_wide_rowmix at rp = 128 over 32771 tiles, one position, per-tile N (4.3 GB): the second launch with its own tiles of
    In, N and Out.  The bound of test_gpu_tile_kernels_wide.test_wide_rowmix, 2^-24 |ref| + n_in 2^-53 (|N|^T |In|); rows
    [n_out, rp) exactly zero; positions from len on and the tiles around Out keep their fill."""
    ctx = gpu_ctx
    rp, n_in, n_out, length = WIDE_RP, 90, 37, 1
    ld_in, ld_out = 4, 6
    rng = np.random.default_rng(12)
    src7 = np.full((PERIOD, rp, ld_in), np.nan, dtype=np.float32)
    src7[:, :n_in, :length] = rng.standard_normal((PERIOD, n_in, length)).astype(np.float32)
    nm7 = np.full((PERIOD, rp, rp), np.nan)
    nm7[:, :n_in, :n_out] = rng.standard_normal((PERIOD, n_in, n_out))
    x64 = src7[:, :n_in, :length].astype(np.float64)
    ref7 = np.einsum("npc,npt->nct", nm7[:, :n_in, :n_out], x64)
    bound7 = U32 * np.abs(ref7) + n_in * U64 * np.einsum("npc,npt->nct", np.abs(nm7[:, :n_in, :n_out]), np.abs(x64))
    ind, nd = expand(ctx, src7, N_TILES), expand(ctx, nm7, N_TILES)
    whole = prefilled(ctx, (GUARD + N_TILES + GUARD, rp, ld_out))
    out = whole[GUARD:GUARD + N_TILES]
    ctx.call("pmdk_wide_rowmix", P(ind), rp * ld_in, ld_in, P(nd), rp * rp, rp, n_in, n_out, P(out), rp * ld_out, ld_out, length,
             N_TILES)
    ctx.sync()
    assert kept(whole[:GUARD]) and kept(whole[GUARD + N_TILES:]) and kept(out[:, :, length:].contiguous()), "fill written"
    assert bool((out[:, n_out:, :length] == 0).all().item()), "rows [n_out, rp) must be zero up to len"
    check_bound(ctx, out[:, :n_out, :length], ref7, bound7, "wide_rowmix")


def test_wide_eig(gpu_ctx):
    """pmdk_wide_eig at rp = 128, order 3, one slice, over 32771 tiles: wide_sym_sum and wide_eig_finish each run in two
    launches around one batched rocSOLVER solve, the second with its own tiles of G, of the workspace, of Nout and of lam.
    Tile t holds the matrix of pattern t % 7 (an antisymmetric part added, NaN outside the leading 3 x 3 block).  The bounds
    of test_gpu_tile_kernels_wide.test_wide_eig in every tile: eigenvalues descending and equal to numpy's to rtol 1e-9 /
    atol 1e-12 lam_max, vectors orthonormal to 1e-12, |M V - V diag(lam)| < 1e-11 lam_max, zeros outside 3 x 3 and beyond the
    order; the tiles around both outputs keep their fill."""
    torch, ctx = _t(), gpu_ctx
    rp, n = WIDE_RP, 3
    rng = np.random.default_rng(13)
    mats = []
    for j in range(PERIOD):
        A = rng.standard_normal((n, 40)) * np.logspace(0, -2, n)[:, None] * (1.0 + j)
        mats.append(A @ A.T)
    mats = np.stack(mats)
    anti = rng.standard_normal((PERIOD, n, n))
    anti = anti - anti.transpose(0, 2, 1)
    g7 = np.full((PERIOD, 1, rp, rp), np.nan)
    g7[:, 0, :n, :n] = mats + anti
    lam7 = np.stack([np.linalg.eigvalsh(m)[::-1] for m in mats])
    Gd = expand(ctx, g7, N_TILES)
    n_whole = prefilled(ctx, (GUARD + N_TILES + GUARD, rp, rp), double=True)
    l_whole = prefilled(ctx, (GUARD + N_TILES + GUARD, rp), double=True)
    Nout, lam = n_whole[GUARD:GUARD + N_TILES], l_whole[GUARD:GUARD + N_TILES]
    nbytes = int(ctx.lib.pmdk_wide_eig_workspace_bytes(n, N_TILES))
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=ctx.device)
    ctx.call("pmdk_wide_eig", P(Gd), 1, rp, n, 0, 0.0, P(Nout), P(lam), N_TILES, P(ws), nbytes)
    ctx.sync()
    for whole in (n_whole, l_whole):
        assert kept(whole[:GUARD]) and kept(whole[GUARD + N_TILES:]), "tiles around an output written"
    idx = pattern_of(ctx, N_TILES)
    L, V = lam[:, :n], Nout[:, :n, :n]
    assert bool((lam[:, n:] == 0).all().item()), "eigenvalues beyond the order"
    outside = torch.ones((rp, rp), dtype=torch.bool, device=ctx.device)
    outside[:n, :n] = False
    assert bool((Nout[:, outside] == 0).all().item()), "entries outside n x n"
    w, M = dev(ctx, lam7)[idx], dev(ctx, mats)[idx]
    w0 = w[:, :1]
    assert bool((L[:, 1:] - L[:, :-1] <= 1e-9 * w0).all().item()), "eigenvalues not descending"
    bad = ~((L - w).abs() <= 1e-9 * w.abs() + 1e-12 * w0)
    assert not bool(bad.any().item()), ("eigenvalues", first_bad(bad))
    eye = torch.eye(n, dtype=torch.float64, device=ctx.device)
    orth = (V.transpose(1, 2) @ V - eye).abs().amax(dim=(1, 2))
    resid = (M @ V - V * L[:, None, :]).abs().amax(dim=(1, 2)) / w0[:, 0]
    print(f"\nwide_eig over {N_TILES} tiles: orthonormality {float(orth.max().item()):.2e}, residual / lam_max {float(resid.max().item()):.2e}")
    assert not bool((~(orth < 1e-12)).any().item()), first_bad(~(orth < 1e-12))
    assert not bool((~(resid < 1e-11)).any().item()), first_bad(~(resid < 1e-11))


# ---------------------------------------------------------------------------------------------- register.hip
FRAME = (12, 12)
N_FRAMES = CUT_TILES + 3
# shifts of the seven patterns: none, whole pixels (a copy), fractions (the bilinear form), one far outside the frame
SHIFTS7 = np.array([(0, 0), (3, -4), (0.5, 0), (0, 0.25), (1.75, -2.5), (-0.125, 0.875), (200, 5)])


def _frames7(src, seed):
    rng = np.random.default_rng(seed)
    shape = (PERIOD,) + FRAME
    if src == "float32":
        return (rng.standard_normal(shape) * 3000).astype(np.float32)
    return rng.integers(0, 65536, shape).astype(np.uint16)


def _as_device_frames(ctx, frames7, n):
    """(n, d1, d2) on the device, uint16 as its int16 bit pattern"""
    return expand(ctx, frames7.view(np.int16) if frames7.dtype == np.uint16 else frames7, n)


@pytest.mark.parametrize("src", ["uint16", "float32"])
def test_shift_apply(gpu_ctx, src):
    """pmd_shift_apply on 32771 frames of 12 x 12 (two launches, the second with its own frames of X and out and its own rows
    of ishift and wts), uint16 to uint16 and float32 to float32, nearest and constant border.  Frame f has the pixels and
    the shift of pattern f % 7.  Bit for bit against register_ref.apply_movie, as test_gpu_register.test_apply_bit_for_bit;
    the padding of every output row and frame and the elements around the array keep their fill."""
    from localmd_amd import register as RG

    torch, ctx = _t(), gpu_ctx
    n, (d1, d2) = N_FRAMES, FRAME
    frames7 = _frames7(src, 21)
    x = _as_device_frames(ctx, frames7, n)
    ish7, wts7 = RG.shift_tables(SHIFTS7)
    ish, wts = expand(ctx, ish7, n), expand(ctx, wts7, n)
    ors, ofs = d2 + 1, d1 * (d2 + 1) + 9
    for border in ("nearest", 123.5):
        mode, fill = RG.check_border(border)
        want7 = register_ref.apply_movie(frames7, SHIFTS7, border, src)
        whole = torch.full((GUARD + n + GUARD, ofs), 77, dtype=x.dtype, device=ctx.device)
        out = whole[GUARD:GUARD + n]
        ctx.call("pmd_shift_apply", P(x), ELEM[src], d1 * d2, d2, n, d1, d2, P(ish), P(wts), mode, fill, P(out), ELEM[src], ofs, ors)
        ctx.sync()
        assert bool((whole[:GUARD] == 77).all().item()) and bool((whole[GUARD + n:] == 77).all().item()), "frames around out written"
        assert bool((out[:, d1 * ors:] == 77).all().item()), "padding behind a frame written"
        img = out[:, :d1 * ors].reshape(n, d1, ors)
        assert bool((img[:, :, d2:] == 77).all().item()), "padding behind a row written"
        got = img[:, :, :d2]
        w7 = want7.view(np.int16) if src == "uint16" else want7
        if src == "float32":
            assert not np.isnan(w7).any()
        check_bits(ctx, got, w7, f"shift_apply {src} {border}")


@pytest.mark.parametrize("src", ["uint16", "float32"])
def test_shift_correlate(gpu_ctx, src):
    """pmd_shift_correlate on 32771 frames of 12 x 12, max shift 2 (the 8 x 8 minimum window), with a workspace for all of
    them: the cap of 32768 frames, not the workspace, ends the first group, and the second group has its own frames of X
    and its own surfaces.  Small integers (pixels 0 .. 15, template -7 .. 7): every surface equals the float64 one bit for
    bit, as in test_gpu_register.test_correlate_small_integers_exactly; the elements around the surfaces keep their fill."""
    torch, ctx = _t(), gpu_ctx
    n, (d1, d2), my, mx = N_FRAMES, FRAME, 2, 2
    ns = (2 * my + 1) * (2 * mx + 1)
    rng = np.random.default_rng(22)
    tp = rng.integers(-7, 8, (d1 - 2 * my, d2 - 2 * mx)).astype(np.float32)
    frames7 = rng.integers(0, 16, (PERIOD,) + FRAME).astype(src)
    want7 = np.stack([register_ref.surface64(f, tp) for f in frames7])
    assert np.abs(want7).max() < 2 ** 24
    x = _as_device_frames(ctx, frames7, n)
    per = int(ctx.lib.pmd_shift_correlate_workspace_bytes(1, d1, d2, my, mx))
    ws_bytes = per * n
    assert ws_bytes // per > CUT_TILES
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=ctx.device)
    td = dev(ctx, tp)
    whole = prefilled(ctx, (GUARD + n + GUARD, ns))
    surf = whole[GUARD:GUARD + n]
    ctx.call("pmd_shift_correlate", P(x), ELEM[src], d1 * d2, d2, 0, 0, n, d1, d2, my, mx, P(td), P(surf), P(ws), ws_bytes)
    ctx.sync()
    assert kept(whole[:GUARD]) and kept(whole[GUARD + n:]), "elements around the surfaces written"
    check_bits(ctx, surf, want7.reshape(PERIOD, ns).astype(np.float32), f"shift_correlate {src}")


# ---------------------------------------------------------------------------------------------- piecewise.hip
@pytest.mark.parametrize("src", ["uint16", "float32"])
def test_warp_apply(gpu_ctx, src):
    """pmd_warp_apply on 32771 frames of 12 x 12 with a 2 x 2 grid of displacements per frame (two launches, the second with
    its own frames of X and out and its own grids), uint16 to uint16 and float32 to float32, nearest and constant border.
    Frame f has the pixels and the grid of pattern f % 7: fractions, whole pixels, one grid far outside the frame.  Bit for
    bit against piecewise_ref.warp_movie, as test_gpu_piecewise.test_warp_bit_for_bit; the padding of every output row and
    frame and the frames around the array keep their fill."""
    from localmd_amd import piecewise as PW
    from localmd_amd import register as RG
    from tests import piecewise_ref

    torch, ctx = _t(), gpu_ctx
    n, (d1, d2), gy, gx = N_FRAMES, FRAME, 2, 2
    frames7 = _frames7(src, 31)
    rng = np.random.default_rng(32)
    grid7 = (rng.standard_normal((PERIOD, gy, gx, 2)) * 2).astype(np.float32)
    grid7[3] *= 30
    grid7[4] = np.rint(grid7[4])
    grid7[5] = (40.25, -80.5)
    tabs = PW.make_tables(([3.5, 8.5], [2.5, 8.5]), d1, d2)
    td = [dev(ctx, t, dt) for t, dt in zip(tabs, (np.int32, np.float32, np.int32, np.float32))]
    x, grid = _as_device_frames(ctx, frames7, n), expand(ctx, grid7, n)
    ors, ofs = d2 + 1, d1 * (d2 + 1) + 9
    for border in ("nearest", 123.5):
        mode, fill = RG.check_border(border)
        want7 = piecewise_ref.warp_movie(frames7, grid7, tabs, border, src)
        whole = torch.full((GUARD + n + GUARD, ofs), 77, dtype=x.dtype, device=ctx.device)
        out = whole[GUARD:GUARD + n]
        ctx.call("pmd_warp_apply", P(x), ELEM[src], d1 * d2, d2, n, d1, d2, P(grid), gy, gx, P(td[0]), P(td[1]), P(td[2]), P(td[3]),
                 mode, fill, P(out), ELEM[src], ofs, ors)
        ctx.sync()
        assert bool((whole[:GUARD] == 77).all().item()) and bool((whole[GUARD + n:] == 77).all().item()), "frames around out written"
        assert bool((out[:, d1 * ors:] == 77).all().item()), "padding behind a frame written"
        img = out[:, :d1 * ors].reshape(n, d1, ors)
        assert bool((img[:, :, d2:] == 77).all().item()), "padding behind a row written"
        w7 = want7.view(np.int16) if src == "uint16" else want7
        if src == "float32":
            assert not np.isnan(w7).any()
        check_bits(ctx, img[:, :, :d2], w7, f"warp_apply {src} {border}")


@pytest.mark.parametrize("src", ["uint16", "float32"])
def test_patch_correlate(gpu_ctx, src):
    """pmd_patch_correlate on 32771 frames of 12 x 12 (max shift 1, deviation 1: one 8 x 8 patch, the smallest the entry
    accepts), with a workspace for all of them: the cap of 32768 frames ends the first group, and the second has its own
    frames of X, its own centres and its own surfaces.  Frame f has the pixels and the centre of pattern f % 7.  Small
    integers: every surface equals the float64 one bit for bit, as in test_gpu_piecewise.test_patch_small_integers_exactly."""
    from tests import piecewise_ref as Q

    torch, ctx = _t(), gpu_ctx
    n, (d1, d2) = N_FRAMES, FRAME
    geo = Q.geometry(d1, d2, (1, 1), (1, 1), (8, 8), (8, 8))
    assert (geo["gy"], geo["gx"], geo["Hh"], geo["Ww"]) == (1, 1, 8, 8)
    ns = 9
    rng = np.random.default_rng(33)
    tps = rng.integers(-7, 8, (1, 8, 8)).astype(np.float32)
    frames7 = rng.integers(0, 16, (PERIOD,) + FRAME).astype(src)
    cen7 = np.array([(0, 0), (1, 1), (-1, -1), (1, -1), (-1, 1), (0, 1), (-1, 0)], dtype=np.int32)
    want7 = np.stack([Q.frame_surfaces64(f, tps, geo, c) for f, c in zip(frames7, cen7)]).reshape(PERIOD, ns)
    assert np.abs(want7).max() < 2 ** 24
    geom = (d1, d2, 1, 1, 1, 1, 8, 8, 1, 1)
    per = int(ctx.lib.pmd_patch_correlate_workspace_bytes(1, *geom))
    ws_bytes = per * n
    assert per > 0 and ws_bytes // per > CUT_TILES
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=ctx.device)
    x, cen = _as_device_frames(ctx, frames7, n), expand(ctx, cen7, n)
    ys, xs, td = dev(ctx, geo["ystart"], np.int32), dev(ctx, geo["xstart"], np.int32), dev(ctx, tps)
    whole = prefilled(ctx, (GUARD + n + GUARD, ns))
    surf = whole[GUARD:GUARD + n]
    ctx.call("pmd_patch_correlate", P(x), ELEM[src], d1 * d2, d2, n, *geom, P(ys), P(xs), P(cen), P(td), P(surf), P(ws), ws_bytes)
    ctx.sync()
    assert kept(whole[:GUARD]) and kept(whole[GUARD + n:]), "elements around the surfaces written"
    check_bits(ctx, surf, want7.astype(np.float32), f"patch_correlate {src}")


# ---------------------------------------------------------------------------------------------- launchers that reject
PMD_ERR_ARG = -2


def _rejected(ctx, entry, args, text):
    """The call returns PMD_ERR_ARG with `text` in pmd_last_error, and launches nothing (the pointers name four floats)."""
    rc = getattr(ctx.lib, entry)(ctx.handle, *args)
    msg = ctx.lib.pmd_last_error(ctx.handle).decode()
    assert rc == PMD_ERR_ARG and text in msg and entry in msg, (entry, rc, msg)
    ctx.sync()


def test_one_past_the_limit_is_rejected(gpu_ctx):
    """The launchers that do not cut a call refuse one item past what a single launch holds, wherever that costs no memory
    (nothing is launched, so the pointers only have to be non-NULL): grid.y above 65535 in pmd_csr_rows_spmm (both kernels)
    and pmd_transpose_affine, more than 65535 blocks of 64 frames in pmd_group_expand, more than 65535 groups of 62 columns
    in pmd_threshold_moments_accumulate, segments (groups) times frame blocks above 2^31 - 1 in pmd_roi_gather and
    pmd_group_project.  The last two with n = 2^31 - 1 frames, 2^25 frame blocks, and 64 segments: exactly 2^31 workgroups,
    and the frame count at which n + 63 no longer fits an int (the block count was formed in int and came out negative,
    which passed the check; it is formed in long now)."""
    torch, ctx = _t(), gpu_ctx
    t = torch.zeros(4, device=ctx.device)
    p = P(t)
    null = P(None)
    cols = 65535 * 256
    _rejected(ctx, "pmd_csr_rows_spmm", [p, p, p, null, 1, p, cols + 1, cols + 1, p, cols + 1], "too many columns in one call")
    _rejected(ctx, "pmd_csr_rows_spmm", [p, p, p, null, 1, p, 4 * cols + 4, 4 * cols + 4, p, 4 * cols + 4], "too many columns in one call")
    _rejected(ctx, "pmd_transpose_affine", [p, 65535 * 32 + 1, 1, 65535 * 32 + 1, null, null, p, 1], "matrix too large for one call")
    n = 65535 * 64 + 1
    _rejected(ctx, "pmd_group_expand", [null, n, n, 1, 1, p, p, 1, p, 0, null, null, null, null, 0, 1, 1, 1, p, 0],
              "too many patches / frames in one call")
    d2 = 65535 * 62 + 1
    _rejected(ctx, "pmd_threshold_moments_accumulate", [p, 0, d2, 1, 1, d2, p, p], "too many columns in one call")
    n = 2 ** 31 - 1                                                 # 2^25 frame blocks of 64; 64 segments: 2^31 workgroups
    _rejected(ctx, "pmd_roi_gather", [p, 0, n, 1, 64, p, p, p, 0, 0, null, p, n, null, 0], "too many segments x frame blocks")
    _rejected(ctx, "pmd_group_project", [p, 0, n, 1, p, p, 64, p, p, p, 0, 0, null, p, n, null, 0], "too many groups x frame blocks")
    assert bool((t == 0).all().item())
