"""Piecewise registration on the GPU (localmd_amd.piecewise, csrc/piecewise.hip).  pmd_patch_correlate against the float64
surface within the forward bound of the kernel's own summation order (tests/piecewise_ref.py: no tuned tolerance), exactly
on small integers, with the same bits however a patch is batched; pmd_shift_peak on the n P patch surfaces; pmd_warp_apply
bit for bit against the NumPy statements; their bad arguments; register_piecewise, apply_field and WarpedMovie end to end
on the planted movies of tests/piecewise_planted.py.  Any NaN matches any NaN (register_ref.same_bits)."""
import ctypes as C
import gc

import numpy as np
import pytest

import localmd_amd
from localmd_amd import decomposition as Dm
from localmd_amd import piecewise as PW
from localmd_amd import register as RG
from localmd_amd._lib import PMDLibraryError, ptr
from localmd_amd.dataset import lazy_data_loader
from tests import piecewise_ref as Q
from tests import register_ref as R
from tests.piecewise_planted import planted, reference, settings

pytestmark = pytest.mark.gpu
Dm.QUIET = True
_ELEM = {"float32": 0, "uint16": 1, "int16": 2}
_FILL = {"float32": np.nan, "uint16": 65535, "int16": -32768}      # paddings of an input: they would show up
POISON = -7777.0                                                    # paddings of an output: they must stay


def _dev(ctx, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _embed(frames, row_stride, extra):
    """The frames with padded rows and frames: (flat array, frame_stride); the padding is _FILL."""
    n, d1, d2 = frames.shape
    fs = d1 * row_stride + extra
    buf = np.full(n * fs + 8, _FILL[frames.dtype.name], dtype=frames.dtype)
    for k in range(n):
        buf[k * fs:k * fs + d1 * row_stride].reshape(d1, row_stride)[:, :d2] = frames[k]
    return buf, fs


def _frames(rng, src, shape):
    if src == "float32":
        return (300.0 + 80.0 * rng.standard_normal(shape)).astype(np.float32)
    if src == "uint16":
        return rng.integers(0, 65536, shape).astype(np.uint16)
    return rng.integers(-32768, 32768, shape).astype(np.int16)


def _geo(d1, d2, ms, md, patch, stride):
    return Q.geometry(d1, d2, ms, md, patch, stride)


def _tight(ph, pw, ms, md):
    """The geometry of a single patch that fills the patch area."""
    return _geo(ph + 2 * (ms[0] + md[0]), pw + 2 * (ms[1] + md[1]), ms, md, (ph, pw), (ph, pw))


def _centres(rng, n, geo):
    c = np.stack([rng.integers(-geo["my"], geo["my"] + 1, n), rng.integers(-geo["mx"], geo["mx"] + 1, n)], axis=1)
    corners = [(geo["my"], geo["mx"]), (-geo["my"], -geo["mx"]), (geo["my"], -geo["mx"]), (-geo["my"], geo["mx"])]
    c[:min(n, 4)] = corners[:n]
    return c.astype(np.int32)


def _patch(ctx, frames, tps, geo, centres, pad=(0, 0), ws_frames=None, ystart=None, xstart=None):
    """pmd_patch_correlate on (n, d1, d2) frames: (n, gy, gx, 2 ey + 1, 2 ex + 1) float32."""
    import torch

    n, d1, d2 = frames.shape
    ys = np.asarray(geo["ystart"] if ystart is None else ystart, dtype=np.int32)
    xs = np.asarray(geo["xstart"] if xstart is None else xstart, dtype=np.int32)
    gy, gx, ey, ex = len(ys), len(xs), geo["ey"], geo["ex"]
    buf, fs = _embed(frames, d2 + pad[0], pad[1])
    ns = (2 * ey + 1) * (2 * ex + 1)
    geom = (d1, d2, geo["my"], geo["mx"], ey, ex, geo["ph"], geo["pw"], gy, gx)
    per = int(ctx.lib.pmd_patch_correlate_workspace_bytes(1, *geom))
    assert per == 4 * gy * gx * -(-geo["ph"] // 32) * -(-geo["pw"] // 64) * ns
    ws_bytes = per * ws_frames if ws_frames else int(ctx.lib.pmd_patch_correlate_workspace_bytes(n, *geom))
    xd, td, cd = _dev(ctx, buf), _dev(ctx, np.ascontiguousarray(tps, dtype=np.float32)), _dev(ctx, centres.astype(np.int32))
    yd, xsd = _dev(ctx, ys), _dev(ctx, xs)
    surf = torch.full((n * gy * gx * ns + 5,), POISON, dtype=torch.float32, device=ctx.device)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=ctx.device)
    ctx.call("pmd_patch_correlate", ptr(xd), _ELEM[frames.dtype.name], fs, d2 + pad[0], n, *geom, ptr(yd), ptr(xsd),
             ptr(cd), ptr(td), ptr(surf), ptr(ws), ws_bytes)
    ctx.sync()
    out = surf.cpu().numpy()
    assert np.all(out[n * gy * gx * ns:] == POISON)
    return out[:n * gy * gx * ns].reshape(n, gy, gx, 2 * ey + 1, 2 * ex + 1)


def _check_surfaces(got, frames, tps, geo, centres, key, frames_to_check=None):
    for k in (range(len(frames)) if frames_to_check is None else frames_to_check):
        for i in range(geo["gy"]):
            for j in range(geo["gx"]):
                tp = tps[i * geo["gx"] + j]
                want = Q.surface64(frames[k], tp, geo, i, j, centres[k])
                bound = Q.forward_bound(frames[k], tp, geo, i, j, centres[k])
                err = np.abs(got[k, i, j].astype(np.float64) - want)
                assert np.all(err <= bound), (key, k, i, j, float((err / bound).max()))


def _template(rng, geo):
    return (300.0 + 80.0 * rng.standard_normal((geo["d1"], geo["d2"]))).astype(np.float32)


# patch rows x columns one below, at and one above the 32 x 64 tile, and every length of the 4-column tail
_EDGES = [(h, w) for h in (31, 32, 33) for w in (63, 64, 65, 66)]


@pytest.mark.parametrize("src", list(_ELEM))
def test_patch_at_the_tile_edges(gpu_ctx, src):
    rng = np.random.default_rng(1)
    for ph, pw in _EDGES + [(8, 8)]:
        geo = _tight(ph, pw, (2, 3), (3, 3))
        frames, tps = _frames(rng, src, (2, geo["d1"], geo["d2"])), Q.packed_templates(_template(rng, geo), geo)
        cen = _centres(rng, 2, geo)
        _check_surfaces(_patch(gpu_ctx, frames, tps, geo, cen), frames, tps, geo, cen, (src, ph, pw))


# (d1, d2, max_shift, max_deviation, patch, stride): deviations 1, 3, 7 and unequal (8 and 16 accumulators a lane; 32, 17 and
# fewer row classes), 1 x 1, 1 x 3 and 3 x 2 patches, overlapping ones, a pulled-back last one, patches of several tiles
_GEOMETRIES = [
    (30, 34, (2, 2), (1, 1), (24, 28), (24, 28)),                      # 1 x 1, deviation 1
    (40, 100, (3, 3), (3, 3), (28, 30), (28, 29)),                     # 1 x 3
    (94, 80, (4, 4), (3, 3), (40, 36), (20, 30)),                      # 3 x 2, overlapping
    (70, 90, (2, 2), (7, 7), (20, 33), (15, 20)),                      # deviation 7: 16 accumulators, 17 row classes
    (64, 80, (5, 3), (2, 5), (24, 30), (17, 19)),                      # unequal, pulled back on both axes
    (64, 80, (3, 5), (7, 1), (30, 24), (30, 13)),
    (110, 170, (4, 4), (3, 3), (70, 140), (30, 16)),                   # 3 x 3 tiles a patch, 2 x 2 patches
    (50, 60, (15, 8), (1, 2), (8, 8), (8, 8)),                         # the 8 x 8 patch, a large rigid range
]


@pytest.mark.parametrize("geom", _GEOMETRIES, ids=lambda g: "{}x{}-{}-{}".format(g[0], g[1], g[3], g[4]))
def test_patch_over_deviations_grids_and_centres(gpu_ctx, geom):
    rng = np.random.default_rng(2)
    geo = _geo(*geom)
    tps = Q.packed_templates(_template(rng, geo), geo)
    for src in _ELEM:
        frames = _frames(rng, src, (5, geo["d1"], geo["d2"]))
        cen = _centres(rng, 5, geo)                                    # (+-my, +-mx) and different in every frame
        _check_surfaces(_patch(gpu_ctx, frames, tps, geo, cen), frames, tps, geo, cen, (geom, src))
    assert (geo["gy"], geo["gx"]) == {0: (1, 1), 1: (1, 3), 2: (3, 2)}.get(_GEOMETRIES.index(geom), (geo["gy"], geo["gx"]))
    if geom[4] != geom[5]:
        assert geo["ystart"][-1] == geo["Hh"] - geo["ph"] and geo["xstart"][-1] == geo["Ww"] - geo["pw"]


def test_patch_strides_counts_groups_and_company(gpu_ctx):
    """Padded strides read the same pixels; n = 1, 2, 65; a (frame, patch) surface has the same bits alone, among other
    patches, inside a batch, at another position of it, and for every size of the launch group."""
    rng = np.random.default_rng(3)
    geo = _geo(60, 84, (3, 4), (3, 2), (20, 30), (14, 21))
    assert (geo["gy"], geo["gx"]) == (3, 3)
    tps = Q.packed_templates(_template(rng, geo), geo)
    for src in _ELEM:
        frames = _frames(rng, src, (65, geo["d1"], geo["d2"]))
        cen = _centres(rng, 65, geo)
        whole = _patch(gpu_ctx, frames, tps, geo, cen)
        _check_surfaces(whole, frames, tps, geo, cen, src, (0, 1, 64))
        for pad in ((3, 0), (9, 7), (1, 1)):
            assert _patch(gpu_ctx, frames[:2], tps, geo, cen[:2], pad).tobytes() == whole[:2].tobytes(), (src, pad)
        assert _patch(gpu_ctx, frames[:1], tps, geo, cen[:1]).tobytes() == whole[:1].tobytes()
        assert _patch(gpu_ctx, frames[40:41], tps, geo, cen[40:41]).tobytes() == whole[40:41].tobytes()
        moved = np.concatenate([frames[30:], frames[:30]]), np.concatenate([cen[30:], cen[:30]])
        assert _patch(gpu_ctx, moved[0], tps, geo, moved[1])[35:].tobytes() == whole[:30].tobytes()
        for g in (1, 7, 64):                                           # 65, 10 and 2 launch groups; one by default
            assert _patch(gpu_ctx, frames, tps, geo, cen, ws_frames=g).tobytes() == whole.tobytes(), (src, g)
        for i, j in ((0, 0), (1, 2), (2, 1)):                          # the patch alone, and in a 1 x 2 row of its own
            p = i * 3 + j
            alone = _patch(gpu_ctx, frames[:3], tps[p:p + 1], geo, cen[:3], ystart=[geo["ystart"][i]],
                           xstart=[geo["xstart"][j]])
            assert alone[:, 0, 0].tobytes() == whole[:3, i, j].tobytes(), (src, i, j)
            pair = _patch(gpu_ctx, frames[:3], tps[[0, p]], geo, cen[:3], ystart=[geo["ystart"][i]],
                          xstart=[geo["xstart"][0], geo["xstart"][j]])
            assert pair[:, 0, 1].tobytes() == whole[:3, i, j].tobytes(), (src, i, j)


def test_patch_small_integers_exactly(gpu_ctx):
    rng = np.random.default_rng(4)
    for geom in ((44, 90, (2, 3), (3, 3), (20, 40), (10, 30)), (70, 100, (3, 3), (7, 7), (40, 70), (40, 70))):
        geo = _geo(*geom)
        tps = rng.integers(-7, 8, (geo["gy"] * geo["gx"], geo["ph"], geo["pw"])).astype(np.float32)
        for src in _ELEM:
            frames = rng.integers(0, 16, (2, geo["d1"], geo["d2"])).astype(src)
            cen = _centres(rng, 2, geo)
            got = _patch(gpu_ctx, frames, tps, geo, cen)
            want = np.stack([Q.frame_surfaces64(f, tps, geo, c) for f, c in zip(frames, cen)])
            assert np.abs(want).max() < 2 ** 24 and np.array_equal(got.astype(np.float64), want), (geom, src)


def test_patch_against_the_rigid_kernel_on_the_sub_image(gpu_ctx):
    """pmd_shift_correlate on the (ph + 2 ey) x (pw + 2 ex) sub-image with max_shift = (ey, ex) computes the same sums in
    another order: the two agree within the sum of both forward bounds."""
    import torch

    rng = np.random.default_rng(5)
    geo = _geo(80, 110, (3, 3), (3, 2), (40, 70), (25, 21))
    tps = Q.packed_templates(_template(rng, geo), geo)
    frames = _frames(rng, "float32", (3, geo["d1"], geo["d2"]))
    cen = _centres(rng, 3, geo)
    got = _patch(gpu_ctx, frames, tps, geo, cen)
    ey, ex, ph, pw = geo["ey"], geo["ex"], geo["ph"], geo["pw"]
    s1, s2 = ph + 2 * ey, pw + 2 * ex
    ws_bytes = int(gpu_ctx.lib.pmd_shift_correlate_workspace_bytes(1, s1, s2, ey, ex))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=gpu_ctx.device)
    surf = torch.empty((2 * ey + 1) * (2 * ex + 1), dtype=torch.float32, device=gpu_ctx.device)
    xd = _dev(gpu_ctx, frames)
    for k in range(3):
        for i in range(geo["gy"]):
            for j in range(geo["gx"]):
                td = _dev(gpu_ctx, tps[i * geo["gx"] + j])
                y0, x0 = geo["my"] + geo["ystart"][i] + cen[k, 0], geo["mx"] + geo["xstart"][j] + cen[k, 1]
                gpu_ctx.call("pmd_shift_correlate", C.c_void_p(xd.data_ptr() + 4 * k * geo["d1"] * geo["d2"]), 0,
                             geo["d1"] * geo["d2"], geo["d2"], int(y0), int(x0), 1, s1, s2, ey, ex, ptr(td), ptr(surf),
                             ptr(ws), ws_bytes)
                gpu_ctx.sync()
                rigid = surf.cpu().numpy().reshape(2 * ey + 1, 2 * ex + 1)
                sub = Q.sub_image(frames[k], geo, i, j, cen[k])
                both = Q.forward_bound(frames[k], tps[i * geo["gx"] + j], geo, i, j, cen[k]) + \
                    R.forward_bound(sub, tps[i * geo["gx"] + j], ey, ex)
                assert np.all(np.abs(rigid.astype(np.float64) - got[k, i, j]) <= both), (k, i, j)


def test_patch_nan_and_inf_pixels(gpu_ctx):
    rng = np.random.default_rng(6)
    geo = _tight(30, 50, (2, 2), (3, 4))
    tps = Q.packed_templates(_template(rng, geo), geo)
    frames = _frames(rng, "float32", (5, geo["d1"], geo["d2"]))
    cen = np.zeros((5, 2), np.int32)
    frames[0, 2, 2] = np.nan                     # the corner of the halo: inside the footprint of one entry only
    frames[1, 20, 30] = np.nan                   # the middle: every entry
    frames[2, 8, 50] = np.inf
    frames[3, 20, 30], frames[3, 21, 31] = np.inf, -np.inf
    frames[4, 0, 0] = np.nan                     # outside every footprint at centre 0: no entry
    got = _patch(gpu_ctx, frames, tps, geo, cen)[:, 0, 0]
    with np.errstate(invalid="ignore"):
        want = np.stack([Q.surface64(f, tps[0], geo, 0, 0, c) for f, c in zip(frames, cen)])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[0]).sum() == 1 and np.isnan(got[0, 0, 0]) and np.isnan(got[1]).all() and not np.isnan(got[4]).any()
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]) and inf.any()
    fin = np.isfinite(want)
    for k in range(5):
        clean = np.where(np.isfinite(frames[k]), frames[k], 0)
        bound = Q.forward_bound(clean, tps[0], geo, 0, 0, cen[k])
        assert np.all(np.abs(got[k][fin[k]].astype(np.float64) - want[k][fin[k]]) <= bound[fin[k]]), k


def test_patch_clamps_centres_and_starts(gpu_ctx):
    """No table can make the kernel read outside the frame: a centre beyond the search range and a start outside the
    patch area give the surface of the clamped value (the frames sit in NaN padding, which would show up)."""
    rng = np.random.default_rng(7)
    geo = _geo(50, 64, (3, 2), (2, 3), (16, 20), (12, 15))
    tps = Q.packed_templates(_template(rng, geo), geo)
    frames = _frames(rng, "float32", (4, geo["d1"], geo["d2"]))
    wild = np.array([(100, -100), (-4, 3), (3, 2 ** 30), (-2 ** 31, 0)], dtype=np.int64).astype(np.int32)
    clamped = np.clip(wild, (-3, -2), (3, 2)).astype(np.int32)
    want = _patch(gpu_ctx, frames, tps, geo, clamped, pad=(5, 40))
    _check_surfaces(want, frames, tps, geo, clamped, "clamped")
    assert _patch(gpu_ctx, frames, tps, geo, wild, pad=(5, 40)).tobytes() == want.tobytes()
    ys, xs = list(geo["ystart"]), list(geo["xstart"])
    bad = _patch(gpu_ctx, frames, tps, geo, clamped, pad=(5, 40), ystart=[-7] + ys[1:-1] + [1000], xstart=[-1] + xs[1:-1] + [2 ** 30])
    assert bad.tobytes() == want.tobytes() and np.all(np.isfinite(bad))


def test_patch_rejects_bad_arguments(gpu_ctx):
    import torch

    d1, d2, my, mx, ey, ex, ph, pw, gy, gx = 40, 48, 2, 3, 2, 1, 12, 16, 2, 2
    ns = 5 * 3
    dev = gpu_ctx.device
    x = torch.zeros(3 * 41 * 50, dtype=torch.float32, device=dev)
    tp = torch.zeros(4 * ph * pw, dtype=torch.float32, device=dev)
    ys, xs = torch.tensor([0, 20], dtype=torch.int32, device=dev), torch.tensor([0, 24], dtype=torch.int32, device=dev)
    cen = torch.zeros((3, 2), dtype=torch.int32, device=dev)
    surf = torch.full((3 * 4 * ns,), 5.0, dtype=torch.float32, device=dev)
    per = 4 * 4 * ns
    ws = torch.empty(3 * per, dtype=torch.uint8, device=dev)
    names = ["X", "elem", "fs", "rs", "n", "d1", "d2", "my", "mx", "ey", "ex", "ph", "pw", "gy", "gx", "ys", "xs", "cen",
             "tp", "surf", "ws", "ws_bytes"]
    good = [ptr(x), 0, 41 * 50, 50, 3, d1, d2, my, mx, ey, ex, ph, pw, gy, gx, ptr(ys), ptr(xs), ptr(cen), ptr(tp),
            ptr(surf), ptr(ws), 3 * per]

    def bad(code, **kw):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        with pytest.raises(PMDLibraryError, match=r"failed \({}\)".format(code)):
            gpu_ctx.call("pmd_patch_correlate", *a)

    for kw in (dict(n=-1), dict(my=0), dict(mx=32), dict(ey=0), dict(ex=0), dict(ey=8), dict(ex=8), dict(ph=7), dict(pw=7),
               dict(ph=33), dict(pw=41), dict(my=16), dict(gy=0), dict(gx=0), dict(gy=65, gx=64), dict(d1=16385),
               dict(elem=3), dict(elem=-1), dict(rs=47), dict(fs=39 * 50 + 47), dict(X=None), dict(ys=None), dict(xs=None),
               dict(cen=None), dict(tp=None), dict(surf=None)):
        bad(-2, **kw)                                                       # PMD_ERR_ARG
    for kw in (dict(ws=None), dict(ws_bytes=per - 1), dict(ws_bytes=0)):
        bad(-3, **kw)                                                       # PMD_ERR_WORKSPACE
    wsb = gpu_ctx.lib.pmd_patch_correlate_workspace_bytes
    assert wsb(0, d1, d2, my, mx, ey, ex, ph, pw, gy, gx) == 0 and wsb(3, d1, d2, my, mx, 8, ex, ph, pw, gy, gx) == 0
    assert wsb(3, d1, d2, my, mx, ey, ex, ph, pw, gy, gx) == 3 * per
    gpu_ctx.call("pmd_patch_correlate", *[0 if k == "n" else v for k, v in zip(names, good)])     # n = 0: nothing
    gpu_ctx.sync()
    assert bool((surf == 5.0).all())
    gpu_ctx.call("pmd_patch_correlate", *good)
    gpu_ctx.sync()
    assert bool((surf == 0).all())


# ---- pmd_shift_peak on the n P surfaces ---------------------------------------------------------------------------
def test_peak_of_the_patch_surfaces(gpu_ctx):
    """The existing peak kernel on the n P surfaces with (my, mx) = (ey, ex): the reference's peaks, a NaN surface included."""
    import torch

    rng = np.random.default_rng(8)
    geo = _geo(60, 70, (3, 3), (3, 2), (20, 24), (14, 16))
    tps = Q.packed_templates(_template(rng, geo), geo)
    frames = _frames(rng, "float32", (3, geo["d1"], geo["d2"]))
    frames[1, 30:34, 30:40] = np.nan                                       # under every entry of the patches that hold it
    cen = _centres(rng, 3, geo)
    surf = _patch(gpu_ctx, frames, tps, geo, cen)
    n = surf.shape[0] * geo["gy"] * geo["gx"]
    flat = surf.reshape(n, 7, 5)
    assert np.isnan(flat).all(axis=(1, 2)).any() and np.isfinite(flat).all(axis=(1, 2)).any()
    arg = torch.full((n + 1, 2), 99, dtype=torch.int32, device=gpu_ctx.device)
    pk = torch.full((n + 1,), POISON, dtype=torch.float32, device=gpu_ctx.device)
    nb = torch.full((n + 1, 9), POISON, dtype=torch.float32, device=gpu_ctx.device)
    sd = _dev(gpu_ctx, flat)
    gpu_ctx.call("pmd_shift_peak", ptr(sd), n, 3, 2, ptr(arg), ptr(pk), ptr(nb))
    gpu_ctx.sync()
    arg, pk, nb = arg.cpu().numpy(), pk.cpu().numpy(), nb.cpu().numpy()
    assert np.all(arg[n] == 99) and pk[n] == POISON
    for k in range(n):
        (dy, dx), p, n9 = R.peak(flat[k])
        assert (int(arg[k, 0]), int(arg[k, 1])) == (dy, dx) and R.same_bits(pk[k], np.float32(p)), k
        assert R.same_bits(nb[k].reshape(3, 3), n9), k


# ---- pmd_warp_apply --------------------------------------------------------------------------------------------------
def _warp(ctx, frames, grid, tabs, border, dst, pad=(0, 0, 0, 0)):
    """pmd_warp_apply; pad = extra elements per input row, input frame, output row, output frame."""
    import torch

    n, d1, d2 = frames.shape
    gy, gx = grid.shape[1:3]
    rs, ors = d2 + pad[0], d2 + pad[2]
    buf, fs = _embed(frames, rs, pad[1])
    ofs = d1 * ors + pad[3]
    mode, fill = RG.check_border(border)
    out = torch.from_numpy(np.full(n * ofs + 3, 77, dtype=dst)).to(ctx.device)
    xd, gd = _dev(ctx, buf), _dev(ctx, np.ascontiguousarray(grid, dtype=np.float32))
    td = [_dev(ctx, np.ascontiguousarray(t, dtype=dt)) for t, dt in zip(tabs, (np.int32, np.float32, np.int32, np.float32))]
    ctx.call("pmd_warp_apply", ptr(xd), _ELEM[frames.dtype.name], fs, rs, n, d1, d2, ptr(gd), gy, gx, ptr(td[0]), ptr(td[1]),
             ptr(td[2]), ptr(td[3]), mode, fill, ptr(out), _ELEM[np.dtype(dst).name], ofs, ors)
    ctx.sync()
    o = out.cpu().numpy()
    got = np.empty((n, d1, d2), dtype=dst)
    rest = [o[n * ofs:]]
    for k in range(n):
        img = o[k * ofs:k * ofs + d1 * ors].reshape(d1, ors)
        got[k] = img[:, :d2]
        rest += [img[:, d2:].reshape(-1), o[k * ofs + d1 * ors:(k + 1) * ofs]]
    assert np.all(np.concatenate(rest) == 77)                         # the padding around out is intact
    return got


def _grid_tables(rng, d1, d2, gy, gx):
    yc = np.sort(rng.choice(np.arange(2, d1 - 2), gy, replace=False)) + 0.5
    xc = np.sort(rng.choice(np.arange(2, d2 - 2), gx, replace=False)) + 0.5
    return PW.make_tables((yc, xc), d1, d2)


@pytest.mark.parametrize("src", list(_ELEM))
@pytest.mark.parametrize("dst", list(_ELEM))
def test_warp_bit_for_bit(gpu_ctx, src, dst):
    rng = np.random.default_rng(9)
    d1, d2 = 37, 70
    for gy, gx in ((1, 1), (2, 2), (5, 5), (1, 5), (2, 1)):
        tabs = _grid_tables(rng, d1, d2, gy, gx)
        frames = _frames(rng, src, (6, d1, d2)) if src != "float32" else (rng.standard_normal((6, d1, d2)) * 3000).astype(np.float32)
        grid = (rng.standard_normal((6, gy, gx, 2)) * 2).astype(np.float32)     # crosses integer boundaries inside a frame
        grid[3] *= 30                                                            # reaches far beyond the frame
        grid[4] = np.rint(grid[4])
        grid[5] = (40.25, -80.5)
        for border in ("nearest", 123.5, -9.0):
            got = _warp(gpu_ctx, frames, grid, tabs, border, dst)
            want = Q.warp_movie(frames, grid, tabs, border, dst)
            for k in range(6):
                assert R.same_bits(got[k], want[k]), (gy, gx, border, k)
    got = _warp(gpu_ctx, frames, grid, tabs, 5.0, dst, pad=(3, 5, 1, 9))
    assert R.same_bits(got, Q.warp_movie(frames, grid, tabs, 5.0, dst))
    for d1, d2 in ((1, 1), (2, 257), (3, 256), (9, 5)):                          # fewer rows than a workgroup takes, two column blocks
        small = np.resize(frames, (2, d1, d2)).copy()
        tabs = PW.make_tables(([0.25 * d1, 0.75 * d1], [0.25 * d2, 0.5 * d2, 0.75 * d2]), d1, d2)
        g = (rng.standard_normal((2, 2, 3, 2)) * 1.5).astype(np.float32)
        assert R.same_bits(_warp(gpu_ctx, small, g, tabs, "nearest", dst), Q.warp_movie(small, g, tabs, "nearest", dst))


def test_warp_uniform_integer_grid_equals_shift_apply(gpu_ctx):
    import torch

    rng = np.random.default_rng(10)
    d1, d2 = 40, 90
    tabs = _grid_tables(rng, d1, d2, 3, 4)
    shifts = np.array([(0, 0), (3, -4), (-3, 4), (31, 31), (-45, 2), (5, 100)], dtype=np.float64)
    grid = np.broadcast_to(shifts[:, None, None, :], (6, 3, 4, 2)).astype(np.float32)
    ish, wts = RG.shift_tables(shifts)
    for src in _ELEM:
        frames = _frames(rng, src, (6, d1, d2))
        for dst in _ELEM:
            for border in ("nearest", 50.0):
                mode, fill = RG.check_border(border)
                out = torch.empty((6, d1, d2), dtype=torch.from_numpy(np.zeros(1, dst)).dtype, device=gpu_ctx.device)
                xd, id_, wd = _dev(gpu_ctx, frames), _dev(gpu_ctx, ish), _dev(gpu_ctx, wts)
                gpu_ctx.call("pmd_shift_apply", ptr(xd), _ELEM[src], d1 * d2, d2, 6, d1, d2, ptr(id_), ptr(wd), mode, fill,
                             ptr(out), _ELEM[dst], d1 * d2, d2)
                gpu_ctx.sync()
                assert _warp(gpu_ctx, frames, grid, tabs, border, dst).tobytes() == out.cpu().numpy().tobytes(), (src, dst, border)


def test_warp_nan_huge_entries_and_wild_tables_stay_in_range(gpu_ctx):
    rng = np.random.default_rng(11)
    d1, d2 = 30, 44
    tabs = _grid_tables(rng, d1, d2, 3, 3)
    frames = _frames(rng, "float32", (5, d1, d2))
    grid = (rng.standard_normal((5, 3, 3, 2)) * 2).astype(np.float32)
    grid[0, 1, 1], grid[1], grid[2, 2, 0], grid[3, 0, 2] = np.nan, 3e38, (-np.inf, 1e30), (np.inf, -3e38)
    for border in ("nearest", 7.0):
        got = _warp(gpu_ctx, frames, grid, tabs, border, "float32", pad=(4, 11, 6, 13))
        assert R.same_bits(got, Q.warp_movie(frames, grid, tabs, border, "float32"))
    # tables that no host layer would make: indices far out of range, not monotone, weights outside [0, 1] and NaN
    ri = rng.integers(-5, 9, d1).astype(np.int32)
    ci = rng.integers(-5, 9, d2).astype(np.int32)
    ri[:3], ci[:3] = (-2 ** 31, 2 ** 31 - 1, 7), (2 ** 31 - 1, -2 ** 31, -1)
    rw, cw = (rng.standard_normal(d1) * 2).astype(np.float32), (rng.standard_normal(d2) * 2).astype(np.float32)
    rw[5], cw[7] = np.nan, np.inf
    wild = (ri, rw, ci, cw)
    for dst in ("float32", "uint16"):
        got = _warp(gpu_ctx, frames, grid, wild, 3.0, dst, pad=(2, 3, 4, 5))
        assert R.same_bits(got, Q.warp_movie(frames, grid, wild, 3.0, dst)), dst


def test_warp_rejects_bad_arguments(gpu_ctx):
    import torch

    d1, d2 = 6, 9
    dev = gpu_ctx.device
    x = torch.zeros(2 * 60, dtype=torch.float32, device=dev)
    out = torch.full((2 * 60,), 4.0, dtype=torch.float32, device=dev)
    grid = torch.zeros((2, 2, 3, 2), dtype=torch.float32, device=dev)
    ri, ci = torch.zeros(d1, dtype=torch.int32, device=dev), torch.zeros(d2, dtype=torch.int32, device=dev)
    rw, cw = torch.zeros(d1, dtype=torch.float32, device=dev), torch.zeros(d2, dtype=torch.float32, device=dev)
    names = ["X", "elem", "fs", "rs", "n", "d1", "d2", "grid", "gy", "gx", "ri", "rw", "ci", "cw", "border", "fill", "out",
             "out_elem", "ofs", "ors"]
    good = [ptr(x), 0, 60, 10, 2, d1, d2, ptr(grid), 2, 3, ptr(ri), ptr(rw), ptr(ci), ptr(cw), 0, 0.0, ptr(out), 0, 60, 10]
    for kw in (dict(n=-1), dict(d1=0), dict(d2=0), dict(d1=16385), dict(elem=3), dict(out_elem=-1), dict(border=2),
               dict(border=-1), dict(rs=8), dict(ors=8), dict(fs=58), dict(ofs=58), dict(gy=0), dict(gx=0), dict(gy=65),
               dict(gx=65), dict(X=None), dict(grid=None), dict(ri=None), dict(rw=None), dict(ci=None), dict(cw=None),
               dict(out=None), dict(out=ptr(x)), dict(out=C.c_void_p(x.data_ptr() + 4 * 30))):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        with pytest.raises(PMDLibraryError, match=r"failed \(-2\)"):
            gpu_ctx.call("pmd_warp_apply", *a)
    gpu_ctx.call("pmd_warp_apply", *[0 if k == "n" else v for k, v in zip(names, good)])
    gpu_ctx.sync()
    assert bool((out == 4.0).all())
    gpu_ctx.call("pmd_warp_apply", *good)
    gpu_ctx.sync()
    o = out.cpu().numpy().reshape(2, 6, 10)
    assert np.all(o[:, :, :9] == 0) and np.all(o[:, :, 9] == 4.0)


# ---- register_piecewise ------------------------------------------------------------------------------------------------
class _Counting(lazy_data_loader):
    """A lazy movie over an array; counts how often every frame is served."""

    def __init__(self, a, fail_after=None):
        self.a, self.fail_after, self.served = a, fail_after, 0
        self.count = np.zeros(len(a), dtype=np.int64)

    dtype = property(lambda self: self.a.dtype)
    shape = property(lambda self: self.a.shape)

    def _compute_at_indices(self, indices):
        idx = np.arange(len(self.a))[indices].reshape(-1)
        self.served += len(idx)
        if self.fail_after is not None and self.served > self.fail_after:
            raise OSError("the disk went away")
        np.add.at(self.count, idx, 1)
        return self.a[idx]


def _device_tables(ctx, mov, base, pg):
    """The peak tables of the rigid and of the patch step from the C entry points themselves."""
    import torch

    T, d1, d2 = mov.shape
    xd = torch.from_numpy(mov.copy()).to(ctx.device)
    est, pest = RG._Estimator(ctx, d1, d2, *pg.max_shift, T), PW._PatchEstimator(ctx, pg, T)
    est.set_template(base)
    pest.set_template(base)
    arg, peak, neigh = est.run(C.c_void_p(xd.data_ptr()), _ELEM[mov.dtype.name], 0, T)
    return (arg, peak, neigh) + pest.run(C.c_void_p(xd.data_ptr()), _ELEM[mov.dtype.name], T, est.arg) + (pest.zero,)


def test_planted_field_against_the_reference(gpu_ctx):
    mov, base, truth = planted("field")
    ref, kw = reference("field"), settings("field")
    T, d1, d2 = mov.shape
    out = np.empty((T, d1, d2), np.float32)
    reg = localmd_amd.register_piecewise(mov, out, template=base, ctx=gpu_ctx, **kw)
    assert np.array_equal(reg.rigid.integer_shifts, ref["rigid"]["integer_shifts"])
    assert np.array_equal(reg.integer_shifts, ref["integer_shifts"]) and not reg.fallback.any()
    pg = PW.PatchGrid(d1, d2, kw["max_shift"], kw["max_deviation"], kw["patch"], kw["stride"])
    assert reg.shifts.shape == (T, pg.gy, pg.gx, 2) and reg.patch == kw["patch"] and reg.max_deviation == kw["max_deviation"]
    assert np.array_equal(reg.centers[0], ref["geometry"]["yc"]) and np.array_equal(reg.starts[1], ref["geometry"]["xstart"])
    # the shifts are the host finish of the device's own peak tables
    arg, peak, neigh, parg, ppk, pnb, zero = _device_tables(gpu_ctx, mov, base, pg)
    rigid = arg + RG.subpixel_peak(neigh)
    sh, ints, fb = PW.finish_patches(rigid, arg, parg, ppk, pnb, zero)
    assert np.array_equal(reg.shifts, sh) and np.array_equal(reg.integer_shifts, ints) and np.array_equal(reg.rigid.shifts, rigid)
    assert R.same_bits(reg.peak, ppk) and R.same_bits(reg.rigid.peak, peak)
    for k in range(T):
        (dy, dx), _, _ = R.peak(ref["surfaces"][k, 1, 2])
        assert tuple(parg[k, 1, 2]) == (dy, dx)
    # the output is the warp of the input by the returned shifts
    tabs = PW.make_tables(reg.centers, d1, d2)
    assert R.same_bits(out, PW.warp_frames(mov, reg.shifts, tabs)) and R.same_bits(out[:3], Q.warp_movie(
        mov[:3], reg.shifts[:3], Q.tables(ref["geometry"])))
    assert R.same_bits(localmd_amd.WarpedMovie(mov, reg)[:], out)
    # the field against the truth: within 1.25 x the float64 reference's error (the surfaces differ by rounding only)
    rtabs = Q.tables(ref["geometry"])
    valid = RG.valid_rect(ref["shifts"].reshape(-1, 2), d1, d2)
    ref_rms = Q.field_rms(np.stack([Q.field32(g.astype(np.float32), rtabs) for g in ref["shifts"]]), truth, valid)
    got_rms = Q.field_rms(np.stack([reg.field(t) for t in range(T)]), truth, valid)
    rigid_rms = Q.field_rms(np.broadcast_to(reg.rigid.shifts[:, None, None, :], truth.shape), truth, valid)
    print("field RMS: device {:.4f} px, reference {:.4f} px, rigid {:.4f} px".format(got_rms, ref_rms, rigid_rms))
    assert got_rms <= 1.25 * ref_rms and got_rms < 0.5 * rigid_rms
    assert reg.valid == RG.valid_rect(reg.shifts.reshape(-1, 2), d1, d2)
    # an explicit template, other borders and output types, integer shifts only
    for subpixel, border, dtype in ((False, 0, None), (True, 250.0, "uint16"), (True, "nearest", "int16")):
        o2 = np.empty((T, d1, d2), np.float32 if dtype is None else dtype)
        r2 = localmd_amd.register_piecewise(mov, o2, template=base, subpixel=subpixel, border=border, dtype=dtype,
                                            ctx=gpu_ctx, **kw)
        assert np.array_equal(r2.integer_shifts, ref["integer_shifts"]) and r2.border == border
        if not subpixel:
            assert np.array_equal(r2.shifts, ref["integer_shifts"])
        else:
            assert np.array_equal(r2.shifts, reg.shifts)
        assert R.same_bits(o2, PW.warp_frames(mov, r2.shifts, tabs, border, dtype))


def test_same_bits_for_every_batch_size_source_and_destination(gpu_ctx, tmp_path, monkeypatch):
    import torch

    mov, base, _ = planted("stream")
    kw = settings("stream")
    T, d1, d2 = mov.shape
    args = dict(template=base, border=100.0, ctx=gpu_ctx, **kw)

    def run(movie, out=None, **more):
        out = np.empty((T, d1, d2), np.float32) if out is None else out
        return localmd_amd.register_piecewise(movie, out, **more, **args), out

    def bits(reg, out):
        return (reg.shifts.tobytes(), reg.peak.tobytes(), reg.rigid.shifts.tobytes(), reg.fallback.tobytes(), out.tobytes())

    reg0, out0 = run(mov)                                              # all frames in one batch
    want = bits(reg0, out0)
    assert np.abs(reg0.integer_shifts - reg0.rigid.integer_shifts[:, None, None, :]).max() >= 1
    pg = PW.PatchGrid(d1, d2, kw["max_shift"], kw["max_deviation"], kw["patch"], kw["stride"])
    geo, tps = _geo(d1, d2, kw["max_shift"], kw["max_deviation"], kw["patch"], kw["stride"]), PW.patch_templates(base, pg)[0]
    for k in range(0, T, 211):                                         # the reference's integers on a sample of frames
        c = reg0.rigid.integer_shifts[k]
        assert tuple(c) == R.peak(R.surface64(mov[k], R.window_template(base, *kw["max_shift"])))[0]
        for i in range(pg.gy):
            for j in range(pg.gx):
                (dy, dx), _, _ = R.peak(Q.surface64(mov[k], tps[i * pg.gx + j], geo, i, j, c))
                assert tuple(reg0.integer_shifts[k, i, j]) == (c[0] + dy, c[1] + dx), (k, i, j)
    for fbs in (7, 64):                                                # whole 1024-frame chunks: two batches
        assert bits(*run(mov, frame_batch_size=fbs)) == want, fbs
    monkeypatch.setattr(PW, "SURFACE_CAP", 4 * pg.P * 25 * 100)        # patch surfaces in sub-blocks of 100 frames
    assert PW.surface_frames(1024, pg) == 100
    assert bits(*run(mov, frame_batch_size=1024)) == want
    monkeypatch.undo()
    np.save(tmp_path / "m.npy", mov)
    sources = {"memmap": np.load(tmp_path / "m.npy", mmap_mode="r"), "device": torch.from_numpy(mov.copy()).to(gpu_ctx.device),
               "lazy": _Counting(mov)}
    for key, src in sources.items():
        assert bits(*run(src, frame_batch_size=1024)) == want, key
    dev = torch.empty((T, d1, d2), dtype=torch.float32, device=gpu_ctx.device)
    run(sources["device"], dev)
    assert dev.cpu().numpy().tobytes() == want[4]
    run(mov, dev.zero_(), frame_batch_size=1024)
    assert dev.cpu().numpy().tobytes() == want[4]
    localmd_amd.register_piecewise(mov, str(tmp_path / "o.npy"), frame_batch_size=1024, **args)
    assert np.load(tmp_path / "o.npy").tobytes() == want[4]
    # the second half on its own, for a second channel; a bare array needs the centres
    second = (mov * np.float32(0.5) + np.float32(3.0)).astype(np.float32)
    tabs = PW.make_tables(reg0.centers, d1, d2)
    got = localmd_amd.apply_field(second, np.empty((T, d1, d2), np.float32), reg0, frame_batch_size=1024, ctx=gpu_ctx)
    assert R.same_bits(got, PW.warp_frames(second, reg0.shifts, tabs, 100.0))
    u16 = np.rint(second).astype(np.uint16)
    localmd_amd.apply_field(u16, dev, reg0.shifts, centers=reg0.centers, border="nearest", ctx=gpu_ctx)
    assert R.same_bits(dev.cpu().numpy(), PW.warp_frames(u16, reg0.shifts, tabs, "nearest"))
    q = localmd_amd.apply_field(second, np.empty((T, d1, d2), np.int16), reg0, dtype="int16", ctx=gpu_ctx)
    assert R.same_bits(q, PW.warp_frames(second, reg0.shifts, tabs, 100.0, "int16"))


def test_movie_reads_built_template_failed_export_and_aliasing(gpu_ctx, tmp_path):
    import torch

    mov, base, _ = planted("stream")
    kw = settings("stream")
    T, d1, d2 = mov.shape
    sample = RG.sample_frames(T, 50)
    dev = torch.empty((T, d1, d2), dtype=torch.float32, device=gpu_ctx.device)
    for out in (None, dev, str(tmp_path / "r.npy")):
        src = _Counting(mov)
        localmd_amd.register_piecewise(src, out, template=base, frame_batch_size=1024, ctx=gpu_ctx, **kw)
        assert np.all(src.count == 1), (type(out), np.unique(src.count))
        src = _Counting(mov)
        reg = localmd_amd.register_piecewise(src, out, template_frames=50, frame_batch_size=1024, ctx=gpu_ctx, **kw)
        want = np.ones(T, np.int64)
        want[sample] += 1                                            # the template's frames in one strided read more
        assert np.array_equal(src.count, want), type(out)
    rig = localmd_amd.register_movie(mov, max_shift=kw["max_shift"], template_frames=50, ctx=gpu_ctx)
    assert reg.template.tobytes() == rig.template.tobytes()          # the template is register_movie's
    assert np.array_equal(reg.rigid.shifts, rig.shifts) and R.same_bits(reg.rigid.peak, rig.peak)
    src = _Counting(mov)
    localmd_amd.apply_field(src, dev, reg, frame_batch_size=1024, ctx=gpu_ctx)
    assert np.all(src.count == 1)
    p = tmp_path / "bad.npy"                                         # a source that fails midway: the file is gone
    with pytest.raises(OSError):
        localmd_amd.register_piecewise(_Counting(mov, fail_after=1100), str(p), template=base, frame_batch_size=1024,
                                       ctx=gpu_ctx, **kw)
    assert not p.exists()
    movd = torch.from_numpy(mov.copy()).to(gpu_ctx.device)
    before = movd.clone()
    for out in (movd, movd[:], movd.view(-1).view(movd.shape)):
        with pytest.raises(ValueError, match="shares memory"):
            localmd_amd.register_piecewise(movd, out, template=base, ctx=gpu_ctx, **kw)
        with pytest.raises(ValueError, match="shares memory"):
            localmd_amd.apply_field(movd, out, reg, ctx=gpu_ctx)
    assert bool((movd == before).all())


def test_device_memory_does_not_grow_with_the_movie(gpu_ctx):
    import torch

    mov, base, _ = planted("stream")
    kw = settings("stream")
    d1, d2 = mov.shape[1:]
    peaks = {}
    for n in (2048, 4096):
        m = np.concatenate([mov] * 4)[:n]
        out = np.empty(m.shape, np.float32)
        gpu_ctx.sync()
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        localmd_amd.register_piecewise(m, out, template=base, frame_batch_size=1024, ctx=gpu_ctx, **kw)
        peaks[n] = torch.cuda.max_memory_allocated() - start
    pg = PW.PatchGrid(d1, d2, kw["max_shift"], kw["max_deviation"], kw["patch"], kw["stride"])
    plan = PW.piecewise_device_bytes(d1=d1, d2=d2, nb=1024, esize=4, host_source=True, n_batches=2, gy=pg.gy, gx=pg.gx, pg=pg,
                                     out_esize=4, host_dest=True)
    assert peaks[4096] <= peaks[2048] + 4096, peaks
    assert 2 * 1024 * d1 * d2 * 4 <= peaks[2048] <= plan, (peaks, plan)


def test_rigid_motion_gives_the_rigid_shift_in_every_patch(gpu_ctx):
    """A movie that moves rigidly: every patch finds the frame's rigid shift within the sub-pixel spread of a parabola
    on a noisy patch, and the output is close to register_movie's."""
    mov, base, truth = planted("rigid")
    kw = settings("rigid")
    T, d1, d2 = mov.shape
    out, rout = np.empty((T, d1, d2), np.float32), np.empty((T, d1, d2), np.float32)
    reg = localmd_amd.register_piecewise(mov, out, template=base, ctx=gpu_ctx, **kw)
    rig = localmd_amd.register_movie(mov, rout, max_shift=kw["max_shift"], template=base, dtype="float32", ctx=gpu_ctx)
    assert np.array_equal(reg.rigid.shifts, rig.shifts) and np.array_equal(rig.integer_shifts, truth[:, 0, 0])
    assert np.array_equal(reg.integer_shifts, np.broadcast_to(rig.integer_shifts[:, None, None, :], reg.integer_shifts.shape))
    ref = reference("rigid")
    ref_spread = np.abs(ref["shifts"] - ref["rigid"]["shifts"][:, None, None, :]).max()
    delta = np.abs(reg.shifts - rig.shifts[:, None, None, :]).max(axis=(1, 2))      # per frame and axis
    print("largest patch shift - rigid shift: device {:.3f} px, float64 reference {:.3f} px".format(delta.max(), ref_spread))
    assert delta.max() <= 1.25 * ref_spread
    # both outputs sample the frame bilinearly, at positions that differ by at most delta (the field is a convex
    # combination of the patch shifts); a bilinear interpolant changes by at most the largest difference of adjacent pixels
    # per pixel moved along an axis
    for k in range(T):
        f = mov[k].astype(np.float64)
        lip = max(np.abs(np.diff(f, axis=0)).max(), np.abs(np.diff(f, axis=1)).max())
        assert np.abs(out[k].astype(np.float64) - rout[k]).max() <= (delta[k].sum() + 1e-4) * lip, k
