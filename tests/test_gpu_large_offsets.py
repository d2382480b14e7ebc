"""
Element offsets past 2^31 and byte offsets past 2^32, reached through a stride (GPU).  Every per-block consumer reads a movie
in blocks of 1024 frames; at 2048 x 2048 pixels that is 4.3 G elements in one call, so a frame, knot or trace row starts
past 2^31 elements although no count in the call is large.  An index formed in 32 bits goes unnoticed at every shape the
other tests use.

One buffer of (2^31 + 2^14) * 4 bytes (8.6 GB) is allocated once for the module with torch.empty and never filled; it is
viewed as uint16, int16 or float32 and is the strided side of a call, the other side a compact tensor of its own.
tests/bigbuf.py has the geometries: three rows (or frames) at stride 2^30 + 4099, the last starting at element
2^31 + 8198, and for each the places a truncated offset would hit instead.  Inputs carry the typed tests' poison there (NaN /
65535 / -32768), so a wrapped read shows in the result; outputs carry a sentinel there, so a wrapped write shows as a
damaged sentinel.  tests/test_bigbuf_host.py checks that arithmetic without a device.  If the buffer cannot be allocated
the module fails; it does not skip.

Comparisons are those of each entry's small test: bit equality for copies, conversions, extrema and sums of small
integers.  No tolerance is new.

Covered: pmd_bin_means (ldy in three types, ldk), pmd_pixel_stats_accumulate, pmd_pixel_hist_accumulate,
pmd_regress_accumulate and pmd_threshold_moments_accumulate (ldy in three types), pmd_baseline_apply (ldx in three types,
ldk, ldo), pmd_sliding_extremum and pmd_sliding_quantile (ldx, ldo), pmd_roi_gather (D = 2^30 + 4099 pixels per frame, uint16
and int16; three float32 frames of that length are 12.9 GB and do not fit the buffer), pmd_roi_combine (ldc, ldr, ldd, lde),
pmd_compact_rows (source, destination), pmd_transpose and pmd_transpose_affine (source, destination), pmd_shift_apply and
pmd_warp_apply (input and output frame stride), pmd_shift_correlate and pmd_patch_correlate (frame stride), the same four
at row_stride = 2^28 + 4099 with the frame stride of 12 such rows (one frame; uint16 and int16: a float32 frame ends at
11.8 GB), pmd_oasis_ar1 (ldy, ldc; T = 2049, as a 2050th row of ldy = 2^20 + 3 would start 1 038 339 elements behind the
buffer's end), pmd_hals_sweep (ldc, ldp).
"""
import numpy as np
import pytest

from tests import bigbuf as B
from tests import register_ref
from tests.device_util import ELEM, PRE32, P, _t, dev

pytestmark = pytest.mark.gpu

TAG = {"float32": "f32", "uint16": "u16", "int16": "i16"}
FILL = {"float32": np.nan, "uint16": 65535, "int16": -32768}      # the poison of an input's alias windows
N, STRIDE = B.ROW_LIVE, B.STRIDE


@pytest.fixture(scope="module")
def big(gpu_ctx):
    """The 8.6 GB buffer as int32 words; freed when the module is done."""
    torch = _t()
    buf = torch.empty(B.WORDS, dtype=torch.int32, device=gpu_ctx.device)
    yield buf
    del buf
    torch.cuda.empty_cache()


def view(big, src):
    """the buffer as the container of `src` (uint16 as its int16 bit pattern)"""
    torch = _t()
    return big.view(torch.float32) if src == "float32" else big.view(torch.int16)


def bits16(a):
    return np.ascontiguousarray(a).view(np.int16) if a.dtype == np.uint16 else a


def put_input(ctx, big, src, geo, rows):
    """rows (len(geo.starts), geo.live) into the live windows, the poison into the alias windows; returns the view"""
    v = view(big, src)
    poison = float("nan") if src == "float32" else int(np.array(FILL[src], dtype=src).view(np.int16))
    for a, b in B.alias_windows(geo):
        v[a:b] = poison
    rows = bits16(np.asarray(rows, dtype=src))
    live = strided(v, geo)
    if live is not None:
        live.copy_(dev(ctx, rows))
    else:
        for (a, b), row in zip(B.live_windows(geo), rows):
            v[a:b] = dev(ctx, row)
    return v


def strided(v, geo):
    """the live windows of `geo` in the view v as one (windows, live) tensor, or None when they are not evenly spaced"""
    steps = np.unique(np.diff(np.asarray(geo.starts)))
    if len(steps) != 1:
        return None
    return _t().as_strided(v, (len(geo.starts), geo.live), (int(steps[0]), 1), int(geo.starts[0]))


def put_sentinel(big, geo):
    """float32 output: the sentinel into live and alias windows; returns the view"""
    v = big.view(_t().float32)
    strided(big, geo).fill_(PRE32)
    for a, b in B.alias_windows(geo):
        big[a:b] = PRE32
    return v


def aliases_kept(big, geo):
    return all(bool((big[a:b] == PRE32).all().item()) for a, b in B.alias_windows(geo))


def live_rows(v, geo):
    return strided(v, geo).cpu().numpy()


def values(rng, src, shape, lo=-30, hi=31):
    """small integers in the container's range: sums and powers of them are exact in fp32, and none is the poison"""
    return rng.integers(max(lo, 0) if src == "uint16" else lo, hi, shape).astype(src)


# ---------------------------------------------------------------------------------------------- baseline.hip, stats.hip
@pytest.mark.parametrize("src", list(ELEM))
def test_bin_means_movie_stride(gpu_ctx, big, src):
    """pmd_bin_means with bin = 1 (K[f] = (float) Y[f], no arithmetic) on three frames at ldy = 2^30 + 4099."""
    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES[f"rows_{TAG[src]}"]
    y = values(np.random.default_rng(1), src, (3, N), -3000, 3000)
    v = put_input(ctx, big, src, geo, y)
    K = torch.full((4, N + 2), -7777.0, device=ctx.device)
    ctx.call("pmd_bin_means", P(v), ELEM[src], STRIDE, 3, N, 0, 1, P(K), N + 2)
    ctx.sync()
    got = K.cpu().numpy()
    assert np.array_equal(got[:3, :N], y.astype(np.float32)), "a frame was read at a truncated offset"
    assert np.all(got[3] == -7777.0) and np.all(got[:, N:] == -7777.0)


def test_bin_means_knot_stride(gpu_ctx, big):
    """The knot rows at ldk = 2^30 + 4099: row 2 is written at element 2^31 + 8198 and nowhere else."""
    ctx = gpu_ctx
    geo = B.GEOMETRIES["rows_f32"]
    y = values(np.random.default_rng(2), "float32", (3, N), -3000, 3000)
    v = put_sentinel(big, geo)
    yd = dev(ctx, y)
    ctx.call("pmd_bin_means", P(yd), 0, N, 3, N, 0, 1, P(v), STRIDE)
    ctx.sync()
    assert aliases_kept(big, geo), "a knot row was written at a truncated offset"
    assert np.array_equal(live_rows(v, geo), y)


@pytest.mark.parametrize("src", list(ELEM))
def test_pixel_stats_movie_stride(gpu_ctx, big, src):
    """pmd_pixel_stats_accumulate with bin = 1 on three frames at ldy = 2^30 + 4099: minimum, maximum, the frames that attain
    them and the four power sums of small integers, all exact."""
    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES[f"rows_{TAG[src]}"]
    y = values(np.random.default_rng(3), src, (3, N))
    v = put_input(ctx, big, src, geo, y)
    ext = torch.empty((2, N), device=ctx.device)
    ext[0], ext[1] = float("inf"), float("-inf")
    arg = torch.full((2, N), -1, dtype=torch.int32, device=ctx.device)
    mom = torch.zeros((4, N), dtype=torch.float64, device=ctx.device)
    ctx.call("pmd_pixel_stats_accumulate", P(v), ELEM[src], STRIDE, 3, N, 0, 1, P(None), P(ext), P(arg), P(mom))
    ctx.sync()
    y64 = y.astype(np.float64)
    assert np.array_equal(ext.cpu().numpy(), np.stack([y64.min(0), y64.max(0)]).astype(np.float32))
    assert np.array_equal(arg.cpu().numpy(), np.stack([y64.argmin(0), y64.argmax(0)]).astype(np.int32))
    assert np.array_equal(mom.cpu().numpy(), np.stack([(y64 ** p).sum(0) for p in (1, 2, 3, 4)]))


# ---------------------------------------------------------------------------------------------- roi.hip
@pytest.mark.parametrize("src", ["uint16", "int16"])
def test_roi_gather_long_frames(gpu_ctx, big, src):
    """pmd_roi_gather on three frames of D = 2^30 + 4099 pixels: ROI j sums eight pixels next to pixel 0, 2^30 and D - 1, so in
    frame 2 every pixel lies past 2^31 elements and in frame 1 two of the three runs do.  Weights 1 .. 3 and small
    integers: exact."""
    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES[f"roi_{TAG[src]}"]
    D, n, p = STRIDE, 3, geo.live
    first = [s for s in geo.starts if s < D]                       # the three runs of frame 0 = their pixel ids
    assert len(first) == 3 and geo.starts == tuple(f * D + c for f in range(n) for c in first)
    rng = np.random.default_rng(4)
    y = values(rng, src, (n, 3, p), -900, 900)                      # [frame][run][pixel]
    v = put_input(ctx, big, src, geo, y.reshape(n * 3, p))
    pix = np.concatenate([np.arange(c, c + p) for c in first]).astype(np.int32)
    wt = rng.integers(1, 4, pix.size).astype(np.float32)
    segs = np.array([[j * p, p, j, 0] for j in range(3)], dtype=np.int64)           # unsplit: straight to row j of out
    out = torch.full((3, n + 1), -7777.0, device=ctx.device)
    sd, pd, wd = dev(ctx, segs), dev(ctx, pix), dev(ctx, wt)
    ctx.call("pmd_roi_gather", P(v), ELEM[src], n, D, 3, P(sd), P(pd), P(wd), 0, 0, P(None), P(out), n + 1, P(None), 0)
    ctx.sync()
    want = np.einsum("jq,fjq->jf", wt.reshape(3, p).astype(np.float64), y.astype(np.float64))
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :n].astype(np.float64), want), "a pixel was read at a truncated offset"
    assert np.all(got[:, n] == -7777.0)


@pytest.mark.parametrize("strided", ["ldc", "ldr", "ldd", "lde"])
def test_roi_combine_strides(gpu_ctx, big, strided):
    """pmd_roi_combine on K = 3 traces of 70 frames with one of its four matrices at a leading dimension of 2^30 + 4099: den =
    C + offset and res = raw - den, the bits of the two fp32 operations in NumPy."""
    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES["traces_f32"]
    rng = np.random.default_rng(5)
    c = (rng.standard_normal((3, N)) * 50).astype(np.float32)
    raw = (rng.standard_normal((3, N)) * 50 + 1000).astype(np.float32)
    off = (1000 + rng.standard_normal(3)).astype(np.float32)
    d = c + off[:, None]
    r = raw - d
    ld = dict(ldc=N, ldr=N, ldd=N, lde=N)
    ld[strided] = STRIDE
    Cd, rawd, offd = dev(ctx, c), dev(ctx, raw), dev(ctx, off)
    den = torch.full((3, N), -7777.0, device=ctx.device)
    res = torch.full((3, N), -7777.0, device=ctx.device)
    if strided == "ldc":
        Cd = put_input(ctx, big, "float32", geo, c)
    elif strided == "ldr":
        rawd = put_input(ctx, big, "float32", geo, raw)
    elif strided == "ldd":
        den = put_sentinel(big, geo)
    else:
        res = put_sentinel(big, geo)
    ctx.call("pmd_roi_combine", 3, N, P(Cd), ld["ldc"], P(offd), P(rawd), ld["ldr"], P(den), ld["ldd"], P(res), ld["lde"])
    ctx.sync()
    if strided in ("ldd", "lde"):
        assert aliases_kept(big, geo), "an output row was written at a truncated offset"
    got_den = live_rows(den, geo) if strided == "ldd" else den.cpu().numpy()
    got_res = live_rows(res, geo) if strided == "lde" else res.cpu().numpy()
    assert np.array_equal(got_den.view(np.int32), d.view(np.int32))
    assert np.array_equal(got_res.view(np.int32), r.view(np.int32))


# ---------------------------------------------------------------------------------------------- gram.hip, global.hip, expand.hip
@pytest.mark.parametrize("strided", ["source", "destination"])
def test_compact_rows_strides(gpu_ctx, big, strided):
    """pmd_compact_rows on one tile of rank 3, T = 70, with ldo (the rows of Out) or ldz (the rows of Z) = 2^30 + 4099: a
    copy, bit for bit."""
    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES["rows_f32"]
    rows = np.random.default_rng(6).standard_normal((3, N)).astype(np.float32)
    ranks, off = dev(ctx, [3], np.int32), dev(ctx, [0], np.int32)
    if strided == "source":
        out = put_input(ctx, big, "float32", geo, rows)
        z = torch.full((4, N + 1), -7777.0, device=ctx.device)
        ctx.call("pmd_compact_rows", P(out), STRIDE, P(off), P(ranks), N, P(z), N + 1, 1)
        ctx.sync()
        got = z.cpu().numpy()
        assert np.array_equal(got[:3, :N].view(np.int32), rows.view(np.int32)), "a row was read at a truncated offset"
        assert np.all(got[3] == -7777.0) and np.all(got[:, N] == -7777.0)
    else:
        out = torch.full((64, N), float("inf"), device=ctx.device)
        out[:3] = dev(ctx, rows)
        z = put_sentinel(big, geo)
        ctx.call("pmd_compact_rows", P(out), N, P(off), P(ranks), N, P(z), STRIDE, 1)
        ctx.sync()
        assert aliases_kept(big, geo), "a row was written at a truncated offset"
        assert np.array_equal(live_rows(z, geo).view(np.int32), rows.view(np.int32))


@pytest.mark.parametrize("strided", ["source", "destination"])
@pytest.mark.parametrize("entry", ["pmd_transpose", "pmd_transpose_affine"])
def test_transpose_strides(gpu_ctx, big, entry, strided):
    """dst[c][r] = src[r][c], for the affine entry times scale[r] = 2 plus shift[r] = 0.5, which is exact on the small integers
    used here; the three long rows are on the strided side, the other matrix is compact."""
    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES["rows_f32"]
    rng = np.random.default_rng(7)
    affine = entry == "pmd_transpose_affine"
    if strided == "source":                                        # src: 3 rows of 70 at lds = 2^30 + 4099 -> dst 70 x 3
        a = rng.integers(-500, 500, (3, N)).astype(np.float32)
        src = put_input(ctx, big, "float32", geo, a)
        dst = torch.full((N + 1, 4), -7777.0, device=ctx.device)
        rows, cols, lds, ldd = 3, N, STRIDE, 4
    else:                                                          # src: 70 x 3 compact -> dst: 3 rows of 70 at ldd = 2^30 + 4099
        a = rng.integers(-500, 500, (N, 3)).astype(np.float32)
        src = dev(ctx, a)
        dst = put_sentinel(big, geo)
        rows, cols, lds, ldd = N, 3, 3, STRIDE
    want = a.T.copy()
    if affine:
        scale = np.full(rows, 2.0, np.float32)
        shift = np.full(rows, 0.5, np.float32)
        want = (a * scale[:, None] + shift[:, None]).T.copy()
        sc, sh = dev(ctx, scale), dev(ctx, shift)
        ctx.call(entry, P(src), lds, rows, cols, P(sc), P(sh), P(dst), ldd)
    else:
        ctx.call(entry, P(src), lds, rows, cols, P(dst), ldd)
    ctx.sync()
    if strided == "source":
        got = dst.cpu().numpy()
        assert np.array_equal(got[:N, :3], want), "a row was read at a truncated offset"
        assert np.all(got[N] == -7777.0) and np.all(got[:, 3] == -7777.0)
    else:
        assert aliases_kept(big, geo), "a row was written at a truncated offset"
        assert np.array_equal(live_rows(dst, geo), want)


# ---------------------------------------------------------------------------------------------- register.hip
SHIFTS = np.array([(0, 0), (1.75, -2.5), (-3, 4)])


@pytest.mark.parametrize("src", list(ELEM))
def test_shift_apply_input_frame_stride(gpu_ctx, big, src):
    """pmd_shift_apply on three frames of 12 x 12 at frame_stride = 2^30 + 4099, to a compact output of the same type: bit for
    bit against register_ref.apply_movie (a copy, a bilinear mix, a whole-pixel shift with the nearest border)."""
    from localmd_amd import register as RG

    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES[f"frames_{TAG[src]}"]
    d1, d2 = B.FRAME
    rng = np.random.default_rng(8)
    frames = values(rng, src, (3, d1, d2), -3000, 3000)
    v = put_input(ctx, big, src, geo, frames.reshape(3, -1))
    ish, wts = RG.shift_tables(SHIFTS)
    ishd, wtsd = dev(ctx, ish), dev(ctx, wts)
    out = torch.full((3, d1 * d2 + 5), 77, dtype=v.dtype, device=ctx.device)
    ctx.call("pmd_shift_apply", P(v), ELEM[src], STRIDE, d2, 3, d1, d2, P(ishd), P(wtsd), 0, 0.0, P(out), ELEM[src], d1 * d2 + 5, d2)
    ctx.sync()
    want = register_ref.apply_movie(frames, SHIFTS, "nearest", src)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :d1 * d2], bits16(want).reshape(3, -1)), "a frame was read at a truncated offset"
    assert np.all(got[:, d1 * d2:] == 77)


def test_shift_apply_output_frame_stride(gpu_ctx, big):
    """The same with the float32 output at out_frame_stride = 2^30 + 4099 and a compact input."""
    from localmd_amd import register as RG

    ctx = gpu_ctx
    geo = B.GEOMETRIES["frames_f32"]
    d1, d2 = B.FRAME
    frames = values(np.random.default_rng(9), "float32", (3, d1, d2), -3000, 3000)
    ish, wts = RG.shift_tables(SHIFTS)
    xd, ishd, wtsd = dev(ctx, frames), dev(ctx, ish), dev(ctx, wts)
    v = put_sentinel(big, geo)
    ctx.call("pmd_shift_apply", P(xd), 0, d1 * d2, d2, 3, d1, d2, P(ishd), P(wtsd), 0, 0.0, P(v), 0, STRIDE, d2)
    ctx.sync()
    assert aliases_kept(big, geo), "a frame was written at a truncated offset"
    want = register_ref.apply_movie(frames, SHIFTS, "nearest", "float32")
    assert np.array_equal(live_rows(v, geo), want.reshape(3, -1))


@pytest.mark.parametrize("src", list(ELEM))
def test_shift_correlate_frame_stride(gpu_ctx, big, src):
    """pmd_shift_correlate on three frames of 12 x 12 at frame_stride = 2^30 + 4099, max shift 2; pixels 0 .. 15 and a template
    of -7 .. 7: every surface equals the float64 one."""
    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES[f"frames_{TAG[src]}"]
    d1, d2 = B.FRAME
    my = mx = 2
    ns = (2 * my + 1) * (2 * mx + 1)
    rng = np.random.default_rng(10)
    tp = rng.integers(-7, 8, (d1 - 2 * my, d2 - 2 * mx)).astype(np.float32)
    frames = rng.integers(0, 16, (3, d1, d2)).astype(src)
    v = put_input(ctx, big, src, geo, frames.reshape(3, -1))
    ws_bytes = int(ctx.lib.pmd_shift_correlate_workspace_bytes(3, d1, d2, my, mx))
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=ctx.device)
    td = dev(ctx, tp)
    surf = torch.full((4, ns), -7777.0, device=ctx.device)
    ctx.call("pmd_shift_correlate", P(v), ELEM[src], STRIDE, d2, 0, 0, 3, d1, d2, my, mx, P(td), P(surf), P(ws), ws_bytes)
    ctx.sync()
    want = np.stack([register_ref.surface64(f, tp) for f in frames]).reshape(3, ns)
    got = surf.cpu().numpy()
    assert np.array_equal(got[:3].astype(np.float64), want), "a frame was read at a truncated offset"
    assert np.all(got[3] == -7777.0)


# ---------------------------------------------------------------------------------------------- baseline.hip: apply, sliding filters
@pytest.mark.parametrize("src", list(ELEM))
def test_baseline_apply_movie_stride(gpu_ctx, big, src):
    """pmd_baseline_apply, mode 1 (x - F0), bin = 1 and T = 3: the knot of frame t is row t of K and F0 is that row without
    arithmetic, so out = (float) X[t] - K[t], one fp32 subtraction of small integers; X at ldx = 2^30 + 4099."""
    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES[f"rows_{TAG[src]}"]
    rng = np.random.default_rng(11)
    x = values(rng, src, (3, N), -3000, 3000)
    k = rng.integers(-500, 500, (3, N)).astype(np.float32)
    v = put_input(ctx, big, src, geo, x)
    kd = dev(ctx, k)
    out = torch.full((4, N + 1), -7777.0, device=ctx.device)
    ctx.call("pmd_baseline_apply", P(v), ELEM[src], STRIDE, 3, N, 0, 3, 1, P(kd), N, 1, 0.0, P(out), N + 1)
    ctx.sync()
    got = out.cpu().numpy()
    assert np.array_equal(got[:3, :N], x.astype(np.float32) - k), "a frame was read at a truncated offset"
    assert np.all(got[3] == -7777.0) and np.all(got[:, N] == -7777.0)


@pytest.mark.parametrize("strided", ["knots", "output"])
def test_baseline_apply_knot_and_output_stride(gpu_ctx, big, strided):
    """Mode 0 (out = F0; X is not read) with bin = 1, T = 3: out[t] = K[t], no arithmetic, with the knot rows (ldk) or the
    output rows (ldo) at 2^30 + 4099."""
    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES["rows_f32"]
    k = np.random.default_rng(12).standard_normal((3, N)).astype(np.float32)
    if strided == "knots":
        kd = put_input(ctx, big, "float32", geo, k)
        out = torch.full((4, N + 1), -7777.0, device=ctx.device)
        ctx.call("pmd_baseline_apply", P(None), 0, N, 3, N, 0, 3, 1, P(kd), STRIDE, 0, 0.0, P(out), N + 1)
        ctx.sync()
        got = out.cpu().numpy()
        assert np.array_equal(got[:3, :N].view(np.int32), k.view(np.int32)), "a knot row was read at a truncated offset"
        assert np.all(got[3] == -7777.0) and np.all(got[:, N] == -7777.0)
    else:
        kd = dev(ctx, k)
        v = put_sentinel(big, geo)
        ctx.call("pmd_baseline_apply", P(None), 0, N, 3, N, 0, 3, 1, P(kd), N, 0, 0.0, P(v), STRIDE)
        ctx.sync()
        assert aliases_kept(big, geo), "an output row was written at a truncated offset"
        assert np.array_equal(live_rows(v, geo).view(np.int32), k.view(np.int32))


def _window_rows(x, half):
    """(n, 2 half + 1, N): the window of every row with the edges replicated"""
    n = x.shape[0]
    return np.stack([x[np.clip(np.arange(j - half, j + half + 1), 0, n - 1)] for j in range(n)])


@pytest.mark.parametrize("strided", ["input", "output"])
@pytest.mark.parametrize("entry", ["pmd_sliding_extremum", "pmd_sliding_quantile"])
def test_sliding_filters_strides(gpu_ctx, big, entry, strided):
    """The sliding minimum (half = 1: a window cut at the edges has the minimum of the replicated one) and the sliding median
    of three rows of small integers, with the rows of X (ldx) or of out (ldo) at 2^30 + 4099: exact."""
    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES["rows_f32"]
    x = values(np.random.default_rng(13), "float32", (3, N), -3000, 3000)
    win = np.sort(_window_rows(x, 1), axis=1)
    want = win[:, 0] if entry == "pmd_sliding_extremum" else win[:, 1]
    if strided == "input":
        xd, ldx = put_input(ctx, big, "float32", geo, x), STRIDE
        out, ldo = torch.full((4, N + 1), -7777.0, device=ctx.device), N + 1
    else:
        xd, ldx = dev(ctx, x), N
        out, ldo = put_sentinel(big, geo), STRIDE
    if entry == "pmd_sliding_extremum":
        nw = int(ctx.lib.pmd_sliding_extremum_work_floats(3, N))
        work = torch.empty(max(nw, 1), device=ctx.device)
        ctx.call(entry, P(xd), ldx, 3, N, 1, 0, P(out), ldo, P(work), nw)
    else:
        nw = int(ctx.lib.pmd_sliding_quantile_work_floats(3, N, 1))
        work = torch.empty(max(nw, 1), device=ctx.device)
        ctx.call(entry, P(xd), ldx, 3, N, 1, 1, P(out), ldo, P(work), nw)
    ctx.sync()
    if strided == "input":
        got = out.cpu().numpy()
        assert np.array_equal(got[:3, :N], want), "a row was read at a truncated offset"
        assert np.all(got[3] == -7777.0) and np.all(got[:, N] == -7777.0)
    else:
        assert aliases_kept(big, geo), "a row was written at a truncated offset"
        assert np.array_equal(live_rows(out, geo), want)


# ---------------------------------------------------------------------------------------------- piecewise.hip
@pytest.mark.parametrize("strided", ["input", "output"])
def test_warp_apply_frame_strides(gpu_ctx, big, strided):
    """pmd_warp_apply on three float32 frames of 12 x 12 with a 2 x 2 grid each, the input or the output frames at a stride of
    2^30 + 4099: bit for bit against piecewise_ref.warp_movie."""
    from localmd_amd import piecewise as PW
    from tests import piecewise_ref

    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES["frames_f32"]
    d1, d2 = B.FRAME
    rng = np.random.default_rng(14)
    frames = values(rng, "float32", (3, d1, d2), -3000, 3000)
    grid = (rng.standard_normal((3, 2, 2, 2)) * 2).astype(np.float32)
    tabs = PW.make_tables(([3.5, 8.5], [2.5, 8.5]), d1, d2)
    td = [dev(ctx, t, dt) for t, dt in zip(tabs, (np.int32, np.float32, np.int32, np.float32))]
    gd = dev(ctx, grid)
    want = piecewise_ref.warp_movie(frames, grid, tabs, "nearest", "float32").reshape(3, -1)
    assert not np.isnan(want).any()
    if strided == "input":
        x, fs = put_input(ctx, big, "float32", geo, frames.reshape(3, -1)), STRIDE
        out, ofs = torch.full((3, d1 * d2 + 5), 77.0, device=ctx.device), d1 * d2 + 5
    else:
        x, fs = dev(ctx, frames), d1 * d2
        out, ofs = put_sentinel(big, geo), STRIDE
    ctx.call("pmd_warp_apply", P(x), 0, fs, d2, 3, d1, d2, P(gd), 2, 2, P(td[0]), P(td[1]), P(td[2]), P(td[3]), 0, 0.0, P(out), 0,
             ofs, d2)
    ctx.sync()
    if strided == "input":
        got = out.cpu().numpy()
        assert np.array_equal(got[:, :d1 * d2].view(np.int32), want.view(np.int32)), "a frame was read at a truncated offset"
        assert np.all(got[:, d1 * d2:] == 77.0)
    else:
        assert aliases_kept(big, geo), "a frame was written at a truncated offset"
        assert np.array_equal(live_rows(out, geo).view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("src", list(ELEM))
def test_patch_correlate_frame_stride(gpu_ctx, big, src):
    """pmd_patch_correlate on three frames of 12 x 12 at frame_stride = 2^30 + 4099 (one 8 x 8 patch, max shift and deviation
    1); pixels 0 .. 15 and a template of -7 .. 7: every surface equals the float64 one."""
    from tests import piecewise_ref as Q

    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES[f"frames_{TAG[src]}"]
    d1, d2 = B.FRAME
    pg = Q.geometry(d1, d2, (1, 1), (1, 1), (8, 8), (8, 8))
    rng = np.random.default_rng(15)
    tps = rng.integers(-7, 8, (1, 8, 8)).astype(np.float32)
    frames = rng.integers(0, 16, (3, d1, d2)).astype(src)
    cen = np.array([(0, 0), (1, -1), (-1, 1)], dtype=np.int32)
    want = np.stack([Q.frame_surfaces64(f, tps, pg, c) for f, c in zip(frames, cen)]).reshape(3, 9)
    v = put_input(ctx, big, src, geo, frames.reshape(3, -1))
    geom = (d1, d2, 1, 1, 1, 1, 8, 8, 1, 1)
    ws_bytes = int(ctx.lib.pmd_patch_correlate_workspace_bytes(3, *geom))
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=ctx.device)
    ys, xs, td, cd = dev(ctx, pg["ystart"], np.int32), dev(ctx, pg["xstart"], np.int32), dev(ctx, tps), dev(ctx, cen)
    surf = torch.full((4, 9), -7777.0, device=ctx.device)
    ctx.call("pmd_patch_correlate", P(v), ELEM[src], STRIDE, d2, 3, *geom, P(ys), P(xs), P(cd), P(td), P(surf), P(ws), ws_bytes)
    ctx.sync()
    got = surf.cpu().numpy()
    assert np.array_equal(got[:3].astype(np.float64), want), "a frame was read at a truncated offset"
    assert np.all(got[3] == -7777.0)


# ---------------------------------------------------------------------------------------------- quantile.hip
@pytest.mark.parametrize("src", list(ELEM))
def test_pixel_hist_movie_stride(gpu_ctx, big, src):
    """pmd_pixel_hist_accumulate, pass 0, on three frames at ldy = 2^30 + 4099: the count of every (pixel, top key byte) against
    the keys formed in NumPy as the header defines them.  The poison has a bin of its own in every type (NaN: 255), so a
    frame read at a truncated offset moves counts."""
    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES[f"rows_{TAG[src]}"]
    y = values(np.random.default_rng(16), src, (3, N), -3000, 3000)
    v = put_input(ctx, big, src, geo, y)
    groups = -(-N // 64)
    hist = torch.zeros((groups, 256, 64), dtype=torch.int32, device=ctx.device)
    ctx.call("pmd_pixel_hist_accumulate", P(v), ELEM[src], STRIDE, 3, N, P(None), 0, P(None), P(hist))
    ctx.sync()
    bits = y.astype(np.float32).view(np.uint32)
    key = np.where(bits >> 31 == 1, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)
    want = np.zeros((groups, 256, 64), dtype=np.int32)
    for f in range(3):
        for c in range(N):
            want[c // 64, key[f, c] >> 24, c % 64] += 1
    poison_key = {"float32": 255, "uint16": (np.float32(65535).view(np.uint32) | 0x80000000) >> 24,
                  "int16": (~np.float32(-32768).view(np.uint32)) >> 24}[src]
    assert want[:, int(poison_key)].sum() == 0, "the poison shares a bin with live values: the test would not see a wrapped read"
    assert np.array_equal(hist.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------- regress.hip, superpixel.hip
@pytest.mark.parametrize("src", list(ELEM))
def test_regress_accumulate_movie_stride(gpu_ctx, big, src):
    """pmd_regress_accumulate on three frames at ldy = 2^30 + 4099 against two time courses, no centring: acc = X Y and the
    sums of y and y^2 per pixel, small integers, exact in fp32 in any order."""
    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES[f"rows_{TAG[src]}"]
    rng = np.random.default_rng(17)
    y = values(rng, src, (3, N))
    x = rng.integers(-5, 6, (2, 3)).astype(np.float32)
    v = put_input(ctx, big, src, geo, y)
    xd = torch.full((2, 4), float("nan"), device=ctx.device)
    xd[:, :3] = dev(ctx, x)
    acc = torch.zeros((2, N + 1), dtype=torch.float64, device=ctx.device)
    acc[:, N] = -7777.0
    mom = torch.zeros((2, N), dtype=torch.float64, device=ctx.device)
    ctx.call("pmd_regress_accumulate", P(v), ELEM[src], STRIDE, 3, N, P(None), P(xd), 4, 2, P(acc), N + 1, P(mom))
    ctx.sync()
    y64 = y.astype(np.float64)
    got = acc.cpu().numpy()
    assert np.array_equal(got[:, :N], x.astype(np.float64) @ y64), "a frame was read at a truncated offset"
    assert np.all(got[:, N] == -7777.0)
    assert np.array_equal(mom.cpu().numpy(), np.stack([y64.sum(0), (y64 * y64).sum(0)]))


@pytest.mark.parametrize("src", list(ELEM))
def test_threshold_moments_movie_stride(gpu_ctx, big, src):
    """pmd_threshold_moments_accumulate on three frames of 7 x 10 pixels at ldy = 2^30 + 4099: the six moments of the rectified
    movie against superpixel_ref (fp64 chains of exact products: bit for bit, as test_gpu_superpixels compares them)."""
    from tests import superpixel_ref

    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES[f"rows_{TAG[src]}"]
    d1, d2 = 7, 10
    assert d1 * d2 == N
    rng = np.random.default_rng(18)
    y = values(rng, src, (3, N))
    thr = rng.integers(-5, 11, N).astype(np.float32)
    v = put_input(ctx, big, src, geo, y)
    td = dev(ctx, thr)
    mom = torch.zeros((6, N), dtype=torch.float64, device=ctx.device)
    ctx.call("pmd_threshold_moments_accumulate", P(v), ELEM[src], STRIDE, 3, d1, d2, P(td), P(mom))
    ctx.sync()
    want = superpixel_ref.moments(superpixel_ref.rectified(y.reshape(3, d1, d2), thr.reshape(d1, d2)))
    assert np.any(want[2:] != 0)
    assert np.array_equal(mom.cpu().numpy().view(np.int64), want.view(np.int64)), "a frame was read at a truncated offset"


# ---------------------------------------------------------------------------------------------- row stride of the registration entries
SHIFT1 = np.array([(1.75, -2.5)])


def _image_rows(ctx, big, src, seed, lo, hi):
    """One 12 x 12 frame whose rows lie 2^28 + 4099 elements apart in the buffer: (view, frame (1, 12, 12), geometry)"""
    geo = B.GEOMETRIES[f"imgrows_{TAG[src]}"]
    frame = values(np.random.default_rng(seed), src, (1,) + B.FRAME, lo, hi)
    return put_input(ctx, big, src, geo, frame[0]), frame, geo


@pytest.mark.parametrize("src", ["uint16", "int16"])
def test_shift_correlate_row_stride(gpu_ctx, big, src):
    """pmd_shift_correlate on one frame of 12 x 12 at row_stride = 2^28 + 4099 and the frame stride that goes with it (12 rows):
    rows 8 to 11 start past 2^31 elements.  Small integers: the surface equals the float64 one."""
    ctx, torch = gpu_ctx, _t()
    d1, d2 = B.FRAME
    v, frame, geo = _image_rows(ctx, big, src, 19, 0, 16)
    my = mx = 2
    ns = 25
    tp = np.random.default_rng(20).integers(-7, 8, (d1 - 2 * my, d2 - 2 * mx)).astype(np.float32)
    ws_bytes = int(ctx.lib.pmd_shift_correlate_workspace_bytes(1, d1, d2, my, mx))
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=ctx.device)
    td = dev(ctx, tp)
    surf = torch.full((2, ns), -7777.0, device=ctx.device)
    ctx.call("pmd_shift_correlate", P(v), ELEM[src], d1 * B.ROW_STRIDE, B.ROW_STRIDE, 0, 0, 1, d1, d2, my, mx, P(td), P(surf),
             P(ws), ws_bytes)
    ctx.sync()
    got = surf.cpu().numpy()
    assert np.array_equal(got[0].astype(np.float64), register_ref.surface64(frame[0], tp).reshape(ns)), "a row was read at a truncated offset"
    assert np.all(got[1] == -7777.0)


@pytest.mark.parametrize("src", ["uint16", "int16"])
def test_patch_correlate_row_stride(gpu_ctx, big, src):
    """pmd_patch_correlate on the same frame layout (one 8 x 8 patch, max shift and deviation 1): the surface equals the
    float64 one."""
    from tests import piecewise_ref as Q

    ctx, torch = gpu_ctx, _t()
    d1, d2 = B.FRAME
    v, frame, geo = _image_rows(ctx, big, src, 21, 0, 16)
    pg = Q.geometry(d1, d2, (1, 1), (1, 1), (8, 8), (8, 8))
    tps = np.random.default_rng(22).integers(-7, 8, (1, 8, 8)).astype(np.float32)
    cen = np.array([(1, -1)], dtype=np.int32)
    want = Q.frame_surfaces64(frame[0], tps, pg, cen[0]).reshape(9)
    geom = (d1, d2, 1, 1, 1, 1, 8, 8, 1, 1)
    ws_bytes = int(ctx.lib.pmd_patch_correlate_workspace_bytes(1, *geom))
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=ctx.device)
    ys, xs, td, cd = dev(ctx, pg["ystart"], np.int32), dev(ctx, pg["xstart"], np.int32), dev(ctx, tps), dev(ctx, cen)
    surf = torch.full((2, 9), -7777.0, device=ctx.device)
    ctx.call("pmd_patch_correlate", P(v), ELEM[src], d1 * B.ROW_STRIDE, B.ROW_STRIDE, 1, *geom, P(ys), P(xs), P(cd), P(td), P(surf),
             P(ws), ws_bytes)
    ctx.sync()
    got = surf.cpu().numpy()
    assert np.array_equal(got[0].astype(np.float64), want), "a row was read at a truncated offset"
    assert np.all(got[1] == -7777.0)


@pytest.mark.parametrize("src", ["uint16", "int16"])
@pytest.mark.parametrize("entry", ["pmd_shift_apply", "pmd_warp_apply"])
def test_apply_entries_row_stride(gpu_ctx, big, entry, src):
    """pmd_shift_apply and pmd_warp_apply read one frame of 12 x 12 at row_stride = 2^28 + 4099 and write a compact frame of the
    same type: bit for bit against register_ref.apply_movie / piecewise_ref.warp_movie (a bilinear mix with the nearest
    border, so rows 8 to 11 are read and clamped to)."""
    from localmd_amd import piecewise as PW
    from localmd_amd import register as RG
    from tests import piecewise_ref

    ctx, torch = gpu_ctx, _t()
    d1, d2 = B.FRAME
    v, frame, geo = _image_rows(ctx, big, src, 23, -3000, 3000)
    out = torch.full((1, d1 * d2 + 5), 77, dtype=v.dtype, device=ctx.device)
    fs, rs = d1 * B.ROW_STRIDE, B.ROW_STRIDE
    if entry == "pmd_shift_apply":
        ish, wts = RG.shift_tables(SHIFT1)
        ishd, wtsd = dev(ctx, ish), dev(ctx, wts)
        ctx.call(entry, P(v), ELEM[src], fs, rs, 1, d1, d2, P(ishd), P(wtsd), 0, 0.0, P(out), ELEM[src], d1 * d2 + 5, d2)
        want = register_ref.apply_movie(frame, SHIFT1, "nearest", src)
    else:
        grid = (np.random.default_rng(24).standard_normal((1, 2, 2, 2)) * 2).astype(np.float32)
        tabs = PW.make_tables(([3.5, 8.5], [2.5, 8.5]), d1, d2)
        td = [dev(ctx, t, dt) for t, dt in zip(tabs, (np.int32, np.float32, np.int32, np.float32))]
        gd = dev(ctx, grid)
        ctx.call(entry, P(v), ELEM[src], fs, rs, 1, d1, d2, P(gd), 2, 2, P(td[0]), P(td[1]), P(td[2]), P(td[3]), 0, 0.0, P(out),
                 ELEM[src], d1 * d2 + 5, d2)
        want = piecewise_ref.warp_movie(frame, grid, tabs, "nearest", src)
    ctx.sync()
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :d1 * d2], bits16(want).reshape(1, -1)), "a row was read at a truncated offset"
    assert np.all(got[:, d1 * d2:] == 77)


# ---------------------------------------------------------------------------------------------- oasis.hip
def _oasis_case():
    """Five AR(1) problems of T = 2049 frames (tests/oasis_ref.planted traces), two values of g, soft and hard threshold"""
    from tests import oasis_ref

    T, n = B.OASIS_T, B.OASIS_N
    Y = np.stack([oasis_ref.planted(30 + p, T=T)[0] for p in range(n)], axis=1).astype(np.float32)
    gs = np.array([0.95, 0.9], dtype=np.float32)
    pw = np.stack([oasis_ref.power_table(g, T) for g in gs])
    pw_row = np.array([0, 1, 0, 1, 0], dtype=np.int32)
    par = np.array([[gs[r], lam, s_min, b] for r, lam, s_min, b in
                    zip(pw_row, (0.5, 0.0, 1.0, 0.25, 0.5), (0.0, 0.0, 0.0, 0.3, 0.0), (0.0, 0.1, -0.2, 0.0, 0.05))], dtype=np.float32)
    ref = [oasis_ref.oasis_ar1(Y[:, p], par[p, 0], par[p, 1], par[p, 2], par[p, 3], np.float32, pw[pw_row[p]]) for p in range(n)]
    Ce, Se = np.stack([r[0] for r in ref], axis=1), np.stack([r[1] for r in ref], axis=1)
    return Y, par, pw_row, pw, Ce, Se, np.array([r[2] for r in ref]), np.array([r[3] for r in ref], dtype=np.int32)


@pytest.mark.parametrize("strided_arg", ["ldy", "ldc"])
def test_oasis_ar1_strides(gpu_ctx, big, strided_arg):
    """pmd_oasis_ar1, time-major: T = 2049 frames of five problems with the rows of Y (ldy) or of C (ldc) 2^20 + 3 elements
    apart, so frame 2048 lies past 2^31 elements (a 2050th row would lie behind the buffer).  Calcium, spikes, residual
    sums and pool counts bit for bit against tests/oasis_ref.py, as test_gpu_deconvolve compares them."""
    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES["oasis_f32"]
    T, n, LD = B.OASIS_T, B.OASIS_N, B.OASIS_LD
    Y, par, pw_row, pw, Ce, Se, rss, npl = _oasis_case()
    Sd = torch.full((T, n + 1), float("nan"), device=ctx.device)
    rd = torch.full((n,), float("nan"), dtype=torch.float64, device=ctx.device)
    nd = torch.full((n,), -1, dtype=torch.int32, device=ctx.device)
    if strided_arg == "ldy":
        Yd, ldy = put_input(ctx, big, "float32", geo, Y), LD
        Cd, ldc = torch.full((T, n + 1), float("nan"), device=ctx.device), n + 1
    else:
        Yd, ldy = dev(ctx, Y), n
        Cd, ldc = put_sentinel(big, geo), LD
    nbytes = int(ctx.lib.pmd_oasis_ar1_workspace_bytes(T, n))
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=ctx.device)
    cold, pard = dev(ctx, np.arange(n), np.int32), dev(ctx, par)
    rowd, pwd = dev(ctx, pw_row), dev(ctx, pw, np.float32)
    ctx.call("pmd_oasis_ar1", P(Yd), ldy, T, n, P(cold), P(pard), P(rowd), P(pwd), pw.shape[1], P(Cd), ldc, P(Sd), n + 1, P(rd),
             P(nd), P(ws), nbytes)
    ctx.sync()
    if strided_arg == "ldy":
        c = Cd.cpu().numpy()
        assert np.all(np.isnan(c[:, n])), "the column beyond n_prob was written"
        got_c = c[:, :n]
    else:
        assert aliases_kept(big, geo), "a row of C was written at a truncated offset"
        got_c = live_rows(Cd, geo)
    assert np.array_equal(nd.cpu().numpy(), npl)
    assert np.array_equal(got_c.view(np.int32), Ce.view(np.int32)), "calcium differs: a frame at a truncated offset"
    assert np.array_equal(Sd.cpu().numpy()[:, :n].view(np.int32), Se.view(np.int32))
    assert np.array_equal(rd.cpu().numpy().view(np.int64), rss.view(np.int64))


# ---------------------------------------------------------------------------------------------- hals.hip
@pytest.mark.parametrize("strided_arg", ["ldc", "ldp"])
def test_hals_sweep_strides(gpu_ctx, big, strided_arg):
    """pmd_hals_sweep with K = 3 traces of 70 frames, C (updated in place) or P at a leading dimension of 2^30 + 4099: the bits
    of tests/hals_ref.hals_sweep, as test_gpu_demix compares them; with C in the buffer the places a truncated offset
    would hit keep their poison."""
    from tests import hals_ref

    ctx, torch = gpu_ctx, _t()
    geo = B.GEOMETRIES["traces_f32"]
    rng = np.random.default_rng(25)
    K = 3
    G = np.array([[2.0, 0.5, 0.0], [0.5, 1.5, 0.25], [0.0, 0.25, 1.0]], dtype=np.float32)
    indptr, indices, data = [0], [], []
    for k in range(K):
        nz = np.nonzero(G[k])[0]
        indices += nz.tolist()
        data += G[k, nz].tolist()
        indptr.append(len(indices))
    indptr, indices, data = np.array(indptr, np.int64), np.array(indices, np.int32), np.array(data, np.float32)
    invd = (1.0 / np.diag(G)).astype(np.float32)
    lo = np.array([0.0, -np.inf, 0.0], dtype=np.float32)
    C0 = rng.standard_normal((K, N)).astype(np.float32)
    Pm = rng.standard_normal((K, N)).astype(np.float32)
    want = hals_ref.hals_sweep(C0.copy(), Pm, indptr, indices, data, invd, lo)
    assert (want[0] == 0).any() and (want[1] < 0).any()
    if strided_arg == "ldc":
        Cd, ldc = put_input(ctx, big, "float32", geo, C0), STRIDE
        Pd, ldp = dev(ctx, Pm), N
    else:
        Cd, ldc = dev(ctx, C0), N
        Pd, ldp = put_input(ctx, big, "float32", geo, Pm), STRIDE
    tabs = [dev(ctx, a) for a in (indptr, indices, data, invd, lo)]
    ctx.call("pmd_hals_sweep", P(Cd), ldc, P(Pd), ldp, K, N, *[P(t) for t in tabs])
    ctx.sync()
    if strided_arg == "ldc":
        got = live_rows(Cd, geo)
        v = big.view(torch.float32)
        assert all(bool(torch.isnan(v[a:b]).all().item()) for a, b in B.alias_windows(geo)), "a row of C was written at a truncated offset"
    else:
        got = Cd.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "a row was read or written at a truncated offset"
