"""Rigid registration on the GPU (localmd_amd.register, csrc/register.hip).  pmd_shift_correlate against the float64
surface within the forward bound of the kernel's own summation order (tests/register_ref.py: no tuned tolerance), exactly
on small integers; pmd_shift_peak and pmd_shift_apply bit for bit against the NumPy statements; their bad arguments;
register_movie, apply_shifts and RegisteredMovie end to end on the planted movies of tests/register_planted.py.

"Bit for bit" leaves one thing open: the sign and payload of a NaN that arithmetic produced differ between processors,
so any NaN matches any NaN (register_ref.same_bits)."""
import ctypes as C
import gc

import numpy as np
import pytest

import localmd_amd
from localmd_amd import decomposition as Dm
from localmd_amd import register as RG
from localmd_amd._lib import PMDLibraryError, ptr
from localmd_amd.dataset import TiffArray, lazy_data_loader
from tests import register_ref as R
from tests.register_planted import PLANTED, planted

pytestmark = pytest.mark.gpu
Dm.QUIET = True
_ELEM = {"float32": 0, "uint16": 1, "int16": 2}
_FILL = {"float32": np.nan, "uint16": 65535, "int16": -32768}      # paddings of an input: they would show up
POISON = -7777.0                                                    # paddings of an output: they must stay


def _dev(ctx, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _embed(frames, rows, row_stride, extra, y0, x0):
    """The frames inside a larger allocation: (flat array, frame_stride); everything around them is _FILL."""
    n, d1, d2 = frames.shape
    fs = rows * row_stride + extra
    buf = np.full(n * fs + 8, _FILL[frames.dtype.name], dtype=frames.dtype)
    for k in range(n):
        img = buf[k * fs:k * fs + rows * row_stride].reshape(rows, row_stride)
        img[y0:y0 + d1, x0:x0 + d2] = frames[k]
    return buf, fs


def _correlate(ctx, frames, tp, my, mx, layout=None, ws_frames=None):
    """pmd_shift_correlate on (n, d1, d2) frames; layout = (rows, row_stride, extra, y0, x0) embeds them."""
    import torch

    n, d1, d2 = frames.shape
    rows, rs, extra, y0, x0 = layout or (d1, d2, 0, 0, 0)
    buf, fs = _embed(frames, rows, rs, extra, y0, x0)
    ns = (2 * my + 1) * (2 * mx + 1)
    per = int(ctx.lib.pmd_shift_correlate_workspace_bytes(1, d1, d2, my, mx))
    ws_bytes = per * ws_frames if ws_frames else int(ctx.lib.pmd_shift_correlate_workspace_bytes(n, d1, d2, my, mx))
    assert per == 4 * -(-(d1 - 2 * my) // 32) * -(-(d2 - 2 * mx) // 64) * ns
    xd, td = _dev(ctx, buf), _dev(ctx, np.ascontiguousarray(tp, dtype=np.float32))
    surf = torch.full((n * ns + 5,), POISON, dtype=torch.float32, device=ctx.device)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=ctx.device)
    ctx.call("pmd_shift_correlate", ptr(xd), _ELEM[frames.dtype.name], fs, rs, y0, x0, n, d1, d2, my, mx, ptr(td),
             ptr(surf), ptr(ws), ws_bytes)
    ctx.sync()
    out = surf.cpu().numpy()
    assert np.all(out[n * ns:] == POISON)
    return out[:n * ns].reshape(n, 2 * my + 1, 2 * mx + 1)


def _frames(rng, src, shape):
    if src == "float32":
        return (300.0 + 80.0 * rng.standard_normal(shape)).astype(np.float32)
    if src == "uint16":
        return rng.integers(0, 65536, shape).astype(np.uint16)
    return rng.integers(-32768, 32768, shape).astype(np.int16)


def _template(rng, d1, d2, my, mx):
    return R.window_template(300.0 + 80.0 * rng.standard_normal((d1, d2)), my, mx)


def _check_surfaces(got, frames, tp, my, mx, key):
    for k, f in enumerate(frames):
        want, bound = R.surface64(f, tp), R.forward_bound(f, tp, my, mx)
        err = np.abs(got[k].astype(np.float64) - want)
        assert np.all(err <= bound), (key, k, float((err / bound).max()))


# window rows x columns one below, at and one above the 32 x 64 tile, and every length of the 4-column tail
_EDGES = [(h, w) for h in (31, 32, 33) for w in (63, 64, 65, 66)]
# (d1, d2, my, mx): S = 4, 2, 1 row ranges, one and two chunks, the 8 x 8 minimum, unequal shifts, several tiles
_GEOMETRIES = [(10, 10, 1, 1), (23, 37, 1, 1), (64, 80, 15, 15), (110, 170, 15, 15), (48, 50, 16, 16), (70, 70, 31, 31),
               (102, 132, 31, 31), (40, 90, 3, 20), (90, 40, 20, 3), (60, 61, 9, 15), (75, 140, 31, 4)]


@pytest.mark.parametrize("src", list(_ELEM))
def test_correlate_at_the_tile_edges(gpu_ctx, src):
    rng = np.random.default_rng(1)
    my, mx = 2, 3
    for h, w in _EDGES:
        d1, d2 = h + 2 * my, w + 2 * mx
        frames, tp = _frames(rng, src, (2, d1, d2)), _template(rng, d1, d2, my, mx)
        _check_surfaces(_correlate(gpu_ctx, frames, tp, my, mx), frames, tp, my, mx, (src, h, w))


@pytest.mark.parametrize("m", [15, 31])
def test_correlate_at_the_tile_edges_with_two_and_one_row_ranges(gpu_ctx, m):
    """The same edges where the lanes of a pass fill two waves (max_shift 15: two row ranges) and more than four
    (max_shift 31: one row range, two workgroups per tile)."""
    rng = np.random.default_rng(11)
    for h, w in ((31, 63), (32, 64), (33, 65)):
        d1, d2 = h + 2 * m, w + 2 * m
        for src in _ELEM:
            frames, tp = _frames(rng, src, (2, d1, d2)), _template(rng, d1, d2, m, m)
            _check_surfaces(_correlate(gpu_ctx, frames, tp, m, m), frames, tp, m, m, (src, h, w, m))


@pytest.mark.parametrize("geom", _GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_correlate_over_max_shifts(gpu_ctx, geom):
    d1, d2, my, mx = geom
    rng = np.random.default_rng(2)
    for src in _ELEM:
        frames, tp = _frames(rng, src, (2, d1, d2)), _template(rng, d1, d2, my, mx)
        _check_surfaces(_correlate(gpu_ctx, frames, tp, my, mx), frames, tp, my, mx, (geom, src))


def test_correlate_strides_embedding_counts_and_groups(gpu_ctx):
    """Padded strides and an image inside a larger allocation read the same pixels; n = 1, 2, 65; a frame has the same
    bits alone, inside a batch, at another position of the batch, and for every size of the launch group."""
    rng = np.random.default_rng(3)
    d1, d2, my, mx = 45, 77, 4, 5
    tp = _template(rng, d1, d2, my, mx)
    for src in _ELEM:
        frames = _frames(rng, src, (65, d1, d2))
        whole = _correlate(gpu_ctx, frames, tp, my, mx)
        _check_surfaces(whole[:3], frames[:3], tp, my, mx, src)
        for layout in ((d1, d2 + 3, 0, 0, 0), (d1 + 5, d2 + 9, 7, 2, 4), (d1 + 1, d2 + 1, 1, 1, 1)):
            assert _correlate(gpu_ctx, frames[:2], tp, my, mx, layout).tobytes() == whole[:2].tobytes(), (src, layout)
        assert _correlate(gpu_ctx, frames[:1], tp, my, mx).tobytes() == whole[:1].tobytes()
        assert _correlate(gpu_ctx, frames[40:41], tp, my, mx).tobytes() == whole[40:41].tobytes()
        moved = np.concatenate([frames[30:], frames[:30]])
        assert _correlate(gpu_ctx, moved, tp, my, mx)[35:].tobytes() == whole[:30].tobytes()
        for g in (1, 7, 64):
            assert _correlate(gpu_ctx, frames, tp, my, mx, ws_frames=g).tobytes() == whole.tobytes(), (src, g)


def test_correlate_small_integers_exactly(gpu_ctx):
    rng = np.random.default_rng(4)
    for d1, d2, my, mx in ((37, 71, 2, 3), (70, 140, 15, 15), (80, 90, 31, 4)):
        tp = rng.integers(-7, 8, (d1 - 2 * my, d2 - 2 * mx)).astype(np.float32)
        for src in _ELEM:
            frames = rng.integers(0, 16, (2, d1, d2)).astype(src)
            got = _correlate(gpu_ctx, frames, tp, my, mx)
            want = np.stack([R.surface64(f, tp) for f in frames])
            assert np.abs(want).max() < 2 ** 24 and np.array_equal(got.astype(np.float64), want), (d1, d2, src)


def test_correlate_nan_and_inf_pixels(gpu_ctx):
    rng = np.random.default_rng(5)
    d1, d2, my, mx = 44, 80, 3, 4
    tp = _template(rng, d1, d2, my, mx)
    frames = _frames(rng, "float32", (5, d1, d2))
    frames[0, 0, 0] = np.nan                     # a corner: inside the footprint of one shift only
    frames[1, 20, 40] = np.nan                   # the middle: every shift
    frames[2, 5, 70] = np.inf
    frames[3, 20, 40], frames[3, 21, 41] = np.inf, -np.inf      # both under every shift: inf - inf where the signs agree
    frames[4, 43, 79] = -np.inf
    got = _correlate(gpu_ctx, frames, tp, my, mx)
    with np.errstate(invalid="ignore"):
        want = np.stack([R.surface64(f, tp) for f in frames])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[0]).sum() == 1 and np.isnan(got[0, 0, 0]) and np.isnan(got[1]).all()
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]) and inf.any()
    fin = np.isfinite(want)
    for k in range(5):
        clean = np.where(np.isfinite(frames[k]), frames[k], 0)
        bound = R.forward_bound(clean, tp, my, mx)
        assert np.all(np.abs(got[k][fin[k]].astype(np.float64) - want[k][fin[k]]) <= bound[fin[k]]), k
    assert np.isnan(got[3]).any() and np.isinf(got[3]).any()


def test_correlate_rejects_bad_arguments(gpu_ctx):
    import torch

    d1, d2, my, mx = 20, 24, 2, 3
    ns = 5 * 7
    x = torch.zeros(3 * 21 * 26, dtype=torch.float32, device=gpu_ctx.device)
    tp = torch.zeros(16 * 18, dtype=torch.float32, device=gpu_ctx.device)
    surf = torch.full((3 * ns,), 5.0, dtype=torch.float32, device=gpu_ctx.device)
    per = 4 * ns
    ws = torch.empty(3 * per, dtype=torch.uint8, device=gpu_ctx.device)
    names = ["X", "elem", "fs", "rs", "y0", "x0", "n", "d1", "d2", "my", "mx", "tp", "surf", "ws", "ws_bytes"]
    good = [ptr(x), 0, 21 * 26, 26, 1, 2, 3, d1, d2, my, mx, ptr(tp), ptr(surf), ptr(ws), 3 * per]

    def bad(code, **kw):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        with pytest.raises(PMDLibraryError, match=r"failed \({}\)".format(code)):
            gpu_ctx.call("pmd_shift_correlate", *a)

    for kw in (dict(n=-1), dict(my=0), dict(mx=0), dict(my=32), dict(mx=32), dict(my=7), dict(mx=9), dict(d1=16385),
               dict(elem=3), dict(elem=-1), dict(y0=-1), dict(x0=-1), dict(x0=3), dict(y0=2), dict(rs=23), dict(fs=500),
               dict(X=None), dict(tp=None), dict(surf=None)):
        bad(-2, **kw)                                                       # PMD_ERR_ARG
    for kw in (dict(ws=None), dict(ws_bytes=per - 1), dict(ws_bytes=0)):
        bad(-3, **kw)                                                       # PMD_ERR_WORKSPACE
    assert gpu_ctx.lib.pmd_shift_correlate_workspace_bytes(0, d1, d2, my, mx) == 0
    assert gpu_ctx.lib.pmd_shift_correlate_workspace_bytes(3, d1, d2, 7, mx) == 0
    gpu_ctx.call("pmd_shift_correlate", *[0 if k == "n" else v for k, v in zip(names, good)])     # n = 0: nothing
    gpu_ctx.sync()
    assert bool((surf == 5.0).all())
    gpu_ctx.call("pmd_shift_correlate", *good)
    gpu_ctx.sync()
    assert bool((surf == 0).all())


# ---- pmd_shift_peak ------------------------------------------------------------------------------------------------
def _peak(ctx, surfaces):
    import torch

    s = np.ascontiguousarray(surfaces, dtype=np.float32)
    n, ny, nx = s.shape
    arg = torch.full((n + 1, 2), 99, dtype=torch.int32, device=ctx.device)
    pk = torch.full((n + 1,), POISON, dtype=torch.float32, device=ctx.device)
    nb = torch.full((n + 1, 9), POISON, dtype=torch.float32, device=ctx.device)
    sd = _dev(ctx, s)
    ctx.call("pmd_shift_peak", ptr(sd), n, ny // 2, nx // 2, ptr(arg), ptr(pk), ptr(nb))
    ctx.sync()
    arg, pk, nb = arg.cpu().numpy(), pk.cpu().numpy(), nb.cpu().numpy()
    assert np.all(arg[n] == 99) and pk[n] == POISON and np.all(nb[n] == POISON)
    return arg[:n], pk[:n], nb[:n].reshape(n, 3, 3)


def _check_peaks(ctx, surfaces):
    arg, pk, nb = _peak(ctx, surfaces)
    for k, s in enumerate(np.asarray(surfaces, dtype=np.float32)):
        (dy, dx), p, n9 = R.peak(s)
        assert (int(arg[k, 0]), int(arg[k, 1])) == (dy, dx), k
        assert R.same_bits(pk[k], np.float32(p)) and R.same_bits(nb[k], n9), k
    return arg, pk, nb


def test_peak_ties_edges_corners_and_nan(gpu_ctx):
    rng = np.random.default_rng(6)
    for my, mx in ((1, 1), (4, 7), (15, 15), (31, 31), (31, 2)):
        ny, nx = 2 * my + 1, 2 * mx + 1
        cases = []
        for y, x in ((0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1), (0, mx), (ny - 1, mx), (my, 0), (my, nx - 1),
                     (my, mx)):
            s = rng.standard_normal((ny, nx)).astype(np.float32)
            s[y, x] = 50.0
            cases.append(s)
        ties = np.round(rng.standard_normal((ny, nx)) * 2).astype(np.float32)      # small integers: full of ties
        cases.append(ties)
        flat = np.full((ny, nx), 3.0, np.float32)
        cases.append(flat)
        two = np.zeros((ny, nx), np.float32)
        two[ny - 1, 0] = two[my, nx - 1] = 9.0                                     # 64 lanes apart or not: the first wins
        cases.append(two)
        holes = rng.standard_normal((ny, nx)).astype(np.float32)
        holes[rng.random((ny, nx)) < 0.4] = np.nan
        cases.append(holes)
        top = holes.copy()
        top[np.unravel_index(np.nanargmax(top), top.shape)] = np.nan               # the former winner never wins
        cases.append(top)
        cases.append(np.full((ny, nx), np.nan, np.float32))
        cases.append(np.full((ny, nx), -np.inf, np.float32))
        mixed = np.full((ny, nx), np.nan, np.float32)
        mixed[my, mx] = -np.inf
        cases.append(mixed)
        one = np.full((ny, nx), np.nan, np.float32)
        one[ny - 1, nx - 1] = -3.0
        cases.append(one)
        pinf = rng.standard_normal((ny, nx)).astype(np.float32)
        pinf[my, 0] = np.inf
        cases.append(pinf)
        arg, pk, nb = _check_peaks(gpu_ctx, np.stack(cases))
        assert tuple(arg[0]) == (-my, -mx) and np.isnan(nb[0][0]).all() and np.isnan(nb[0][:, 0]).all()
        assert tuple(arg[10]) == (-my, -mx) and tuple(arg[11]) == (0, mx)
        for k in (14, 15, 16):
            assert tuple(arg[k]) == (0, 0) and np.isnan(pk[k]) and np.isnan(nb[k]).all()
        assert tuple(arg[17]) == (my, mx) and pk[17] == -3.0 and tuple(arg[18]) == (0, -mx) and pk[18] == np.inf


def test_peak_rejects_bad_arguments(gpu_ctx):
    import torch

    s = torch.zeros((2, 5, 7), dtype=torch.float32, device=gpu_ctx.device)
    arg = torch.full((2, 2), 9, dtype=torch.int32, device=gpu_ctx.device)
    pk = torch.zeros(2, dtype=torch.float32, device=gpu_ctx.device)
    nb = torch.zeros(18, dtype=torch.float32, device=gpu_ctx.device)
    good = [ptr(s), 2, 2, 3, ptr(arg), ptr(pk), ptr(nb)]
    for i, v in ((1, -1), (2, 0), (2, 32), (3, 0), (3, 32), (0, None), (4, None), (5, None), (6, None)):
        a = list(good)
        a[i] = v
        with pytest.raises(PMDLibraryError, match=r"failed \(-2\)"):
            gpu_ctx.call("pmd_shift_peak", *a)
    a = list(good)
    a[1] = 0
    gpu_ctx.call("pmd_shift_peak", *a)
    gpu_ctx.sync()
    assert bool((arg == 9).all())
    gpu_ctx.call("pmd_shift_peak", *good)
    gpu_ctx.sync()
    assert bool((arg == torch.tensor([[-2, -3], [-2, -3]], dtype=torch.int32, device=gpu_ctx.device)).all())


# ---- pmd_shift_apply -----------------------------------------------------------------------------------------------
def _apply(ctx, frames, shifts, border, dst, pad=(0, 0, 0, 0)):
    """pmd_shift_apply; pad = extra elements per input row, input frame, output row, output frame."""
    import torch

    n, d1, d2 = frames.shape
    rs, ors = d2 + pad[0], d2 + pad[2]
    buf, fs = _embed(frames, d1, rs, pad[1], 0, 0)
    ofs = d1 * ors + pad[3]
    ish, wts = RG.shift_tables(shifts)
    mode, fill = RG.check_border(border)
    tdt = torch.from_numpy(np.zeros(1, dst)).dtype
    out = torch.from_numpy(np.full(n * ofs + 3, 77, dtype=dst)).to(ctx.device)
    xd, ishd, wtsd = _dev(ctx, buf), _dev(ctx, ish), _dev(ctx, wts)      # kept alive until the kernel has run
    ctx.call("pmd_shift_apply", ptr(xd), _ELEM[frames.dtype.name], fs, rs, n, d1, d2, ptr(ishd), ptr(wtsd), mode, fill,
             ptr(out), _ELEM[np.dtype(dst).name], ofs, ors)
    ctx.sync()
    assert out.dtype == tdt
    o = out.cpu().numpy()
    got = np.empty((n, d1, d2), dtype=dst)
    rest = [o[n * ofs:]]
    for k in range(n):
        img = o[k * ofs:k * ofs + d1 * ors].reshape(d1, ors)
        got[k] = img[:, :d2]
        rest += [img[:, d2:].reshape(-1), o[k * ofs + d1 * ors:(k + 1) * ofs]]
    assert np.all(np.concatenate(rest) == 77)
    return got


_SHIFTS = np.array([(0, 0), (3, -4), (-3, 4), (31, 31), (-31, -31), (200, 5), (-5, -300), (0.5, 0), (0, 0.25),
                    (1.75, -2.5), (-0.125, 0.875), (30.5, -30.5), (150.5, 0.5), (-1e6, 1e6), (2.0 ** 30, -2.0 ** 30)])


@pytest.mark.parametrize("src", list(_ELEM))
@pytest.mark.parametrize("dst", list(_ELEM))
def test_apply_bit_for_bit(gpu_ctx, src, dst):
    rng = np.random.default_rng(7)
    d1, d2 = 37, 70
    if src == "float32":
        frames = (rng.standard_normal((len(_SHIFTS), d1, d2)) * 3000).astype(np.float32)
    else:
        frames = _frames(rng, src, (len(_SHIFTS), d1, d2))
    for border in ("nearest", 123.5, -9.0):
        got = _apply(gpu_ctx, frames, _SHIFTS, border, dst)
        want = R.apply_movie(frames, _SHIFTS, border, dst)
        for k in range(len(_SHIFTS)):
            assert R.same_bits(got[k], want[k]), (border, k, _SHIFTS[k])
    got = _apply(gpu_ctx, frames, _SHIFTS, 5.0, dst, pad=(3, 5, 1, 9))
    assert R.same_bits(got, R.apply_movie(frames, _SHIFTS, 5.0, dst))
    for d1, d2 in ((1, 1), (2, 257), (3, 256)):
        small = frames[:4, :d1, :d2].copy() if d2 <= 70 else np.tile(frames[:4, :d1], (1, 1, 4))[:, :, :d2].copy()
        sh = np.array([(0, 0), (0.5, 0.5), (-1, 1), (0.25, -0.75)])
        assert R.same_bits(_apply(gpu_ctx, small, sh, "nearest", dst), R.apply_movie(small, sh, "nearest", dst))


def test_apply_copies_inf_and_nan_of_integer_shifts(gpu_ctx):
    rng = np.random.default_rng(8)
    frames = rng.standard_normal((4, 20, 33)).astype(np.float32)
    frames[:, 3, 4], frames[:, 10, 10], frames[:, 19, 32] = np.inf, np.nan, -np.inf
    frames[1].view(np.uint32)[10, 11] = 0x7FC12345                  # a NaN with a payload: copied, not computed
    sh = np.array([(0, 0), (2, -3), (-4, 1), (1, 0)], dtype=np.float64)
    got = _apply(gpu_ctx, frames, sh, "nearest", "float32")
    assert got.tobytes() == R.apply_movie(frames, sh, "nearest", "float32").tobytes()      # payloads included
    assert np.isnan(got).sum(axis=(1, 2)).tolist() == [1, 2, 1, 1]
    frac = sh + 0.5                                                  # bilinear: 0 inf never arises from zero weights here
    got = _apply(gpu_ctx, frames, frac, -1.0, "float32")
    assert R.same_bits(got, R.apply_movie(frames, frac, -1.0, "float32"))
    half = np.array([(0, 0.5)] * 4)                                  # w10 = w11 = 0 next to an inf row: 0 inf = NaN, as stated
    assert R.same_bits(_apply(gpu_ctx, frames, half, "nearest", "float32"), R.apply_movie(frames, half, "nearest", "float32"))


def test_apply_rejects_bad_arguments(gpu_ctx):
    import torch

    d1, d2 = 6, 9
    x = torch.zeros(2 * 60, dtype=torch.float32, device=gpu_ctx.device)
    out = torch.full((2 * 60,), 4.0, dtype=torch.float32, device=gpu_ctx.device)
    ish = torch.zeros((2, 2), dtype=torch.int32, device=gpu_ctx.device)
    wts = torch.tensor([[1.0, 0, 0, 0]] * 2, dtype=torch.float32, device=gpu_ctx.device)
    names = ["X", "elem", "fs", "rs", "n", "d1", "d2", "ish", "wts", "border", "fill", "out", "out_elem", "ofs", "ors"]
    good = [ptr(x), 0, 60, 10, 2, d1, d2, ptr(ish), ptr(wts), 0, 0.0, ptr(out), 0, 60, 10]
    for kw in (dict(n=-1), dict(d1=0), dict(d2=0), dict(d1=16385), dict(elem=3), dict(out_elem=-1), dict(border=2),
               dict(border=-1), dict(rs=8), dict(ors=8), dict(fs=58), dict(ofs=58), dict(X=None), dict(ish=None),
               dict(wts=None), dict(out=None), dict(out=ptr(x)), dict(out=C.c_void_p(x.data_ptr() + 4 * 30))):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        with pytest.raises(PMDLibraryError, match=r"failed \(-2\)"):
            gpu_ctx.call("pmd_shift_apply", *a)
    gpu_ctx.call("pmd_shift_apply", *[0 if k == "n" else v for k, v in zip(names, good)])
    gpu_ctx.sync()
    assert bool((out == 4.0).all())
    gpu_ctx.call("pmd_shift_apply", *good)
    gpu_ctx.sync()
    o = out.cpu().numpy().reshape(2, 6, 10)
    assert np.all(o[:, :, :9] == 0) and np.all(o[:, :, 9] == 4.0)


# ---- register_movie ------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("name", ["small", "u16"])
def test_planted_shifts_and_the_reference_on_the_devices_surfaces(gpu_ctx, name):
    mov, base, shifts = planted(name)
    ms = PLANTED[name]["max_shift"]
    T, d1, d2 = mov.shape
    reg = localmd_amd.register_movie(mov, max_shift=ms, template=base, subpixel=False, ctx=gpu_ctx)
    assert np.array_equal(reg.integer_shifts, shifts.astype(np.int32)) and np.array_equal(reg.shifts, shifts)
    assert reg.max_shift == ms and reg.template.tobytes() == base.tobytes() and reg.surfaces is None
    assert set(reg.at_limit.tolist()) == set(np.nonzero((np.abs(shifts) == np.array(ms)).any(axis=1))[0].tolist())
    assert reg.valid == (ms[0], d1 - ms[0], ms[1], d2 - ms[1])
    for subpixel, border, dtype in ((True, "nearest", None), (False, 0, None), (True, 250.0, "uint16"),
                                    (False, "nearest", "float32")):
        out = np.empty((T, d1, d2), RG._resolve_dtype(dtype, mov.dtype, not subpixel))
        reg = localmd_amd.register_movie(mov, out, max_shift=ms, template=base, subpixel=subpixel, border=border,
                                         dtype=dtype, return_surfaces=True, ctx=gpu_ctx)
        assert reg.surfaces.shape == (T, 2 * ms[0] + 1, 2 * ms[1] + 1) and reg.surfaces.dtype == np.float32
        ref = R.register_ref(mov, base, ms, subpixel, border, out.dtype, surfaces=reg.surfaces)
        assert np.array_equal(reg.shifts, ref["shifts"]) and np.array_equal(reg.integer_shifts, ref["integer_shifts"])
        assert R.same_bits(reg.peak, ref["peak"].astype(np.float32)) and R.same_bits(out, ref["movie"])
        assert np.array_equal(reg.integer_shifts, shifts.astype(np.int32))
        tp = R.window_template(base, *ms)
        _check_surfaces(reg.surfaces[:4], mov[:4], tp, ms[0], ms[1], name)
        if subpixel:
            assert np.abs(reg.shifts - shifts).max() <= 0.5 and np.any(reg.shifts != shifts)
        rm = RG.RegisteredMovie(mov, reg, dtype=dtype)
        assert rm.dtype == out.dtype and R.same_bits(rm[:], out)


def test_same_bits_for_every_batch_size_source_and_destination(gpu_ctx, tmp_path):
    import torch
    from localmd_amd._minitiff import TiffWriter

    mov, base, shifts = planted("stream")
    ms = PLANTED["stream"]["max_shift"]
    T, d1, d2 = mov.shape
    kw = dict(max_shift=ms, template=base, border=100.0, ctx=gpu_ctx)

    def run(movie, out=None, **more):
        out = np.empty((T, d1, d2), np.float32) if out is None else out
        reg = localmd_amd.register_movie(movie, out, **more, **kw)
        return reg, out

    reg0, out0 = run(mov, frame_batch_size=10000)
    assert np.array_equal(reg0.integer_shifts, shifts.astype(np.int32))
    want = (reg0.shifts.tobytes(), reg0.peak.tobytes(), out0.tobytes())
    for fbs in (1024, 2048):
        reg, out = run(mov, frame_batch_size=fbs)
        assert (reg.shifts.tobytes(), reg.peak.tobytes(), out.tobytes()) == want, fbs
    np.save(tmp_path / "m.npy", mov)
    with TiffWriter(str(tmp_path / "m.tif"), mov.shape, np.float32) as w:
        w.write(mov)
    sources = {"memmap": np.load(tmp_path / "m.npy", mmap_mode="r"), "tiff": TiffArray(str(tmp_path / "m.tif")),
               "cpu": torch.from_numpy(mov.copy()), "device": torch.from_numpy(mov.copy()).to(gpu_ctx.device),
               "lazy": _Counting(mov)}
    for key, src in sources.items():
        reg, out = run(src, frame_batch_size=1024)
        assert (reg.shifts.tobytes(), reg.peak.tobytes(), out.tobytes()) == want, key
    dev = torch.empty((T, d1, d2), dtype=torch.float32, device=gpu_ctx.device)
    run(sources["device"], dev)
    assert dev.cpu().numpy().tobytes() == want[2]
    run(mov, dev.zero_(), frame_batch_size=1024)
    assert dev.cpu().numpy().tobytes() == want[2]
    cpu = torch.empty((T, d1, d2), dtype=torch.float32)
    run(mov, cpu)
    assert cpu.numpy().tobytes() == want[2]
    localmd_amd.register_movie(mov, str(tmp_path / "o.npy"), frame_batch_size=1024, **kw)
    assert np.load(tmp_path / "o.npy").tobytes() == want[2]
    localmd_amd.register_movie(mov, str(tmp_path / "o.tif"), **kw)
    assert TiffArray(str(tmp_path / "o.tif"))[:].tobytes() == want[2]
    # the second half on its own, for a second channel
    second = (mov * np.float32(0.5) + np.float32(3.0)).astype(np.float32)
    got = localmd_amd.apply_shifts(second, np.empty((T, d1, d2), np.float32), reg0, border=100.0, frame_batch_size=1024,
                                   ctx=gpu_ctx)
    assert R.same_bits(got, R.apply_movie(second, reg0.shifts, 100.0, np.float32))
    whole = localmd_amd.apply_shifts(second.astype(np.int16), np.empty((T, d1, d2), np.int16), shifts, ctx=gpu_ctx)
    assert whole.tobytes() == R.apply_movie(second.astype(np.int16), shifts).tobytes()


def test_movie_reads_template_and_failed_export(gpu_ctx, tmp_path):
    import torch

    mov, base, shifts = planted("stream")
    ms = PLANTED["stream"]["max_shift"]
    T, d1, d2 = mov.shape
    sample = RG.sample_frames(T, 50)
    dev = torch.empty((T, d1, d2), dtype=torch.float32, device=gpu_ctx.device)
    for out in (None, dev, np.empty((T, d1, d2), np.float32), str(tmp_path / "r.npy")):
        src = _Counting(mov)
        localmd_amd.register_movie(src, out, max_shift=ms, template=base, frame_batch_size=1024, ctx=gpu_ctx)
        assert np.all(src.count == 1), (type(out), np.unique(src.count))
        src = _Counting(mov)
        reg = localmd_amd.register_movie(src, out, max_shift=ms, template_frames=50, frame_batch_size=1024, ctx=gpu_ctx)
        want = np.ones(T, np.int64)
        want[sample] += 1                                            # the template's frames in one strided read more
        assert np.array_equal(src.count, want), type(out)
    # the built template: the shifts differ from the planted ones by one common offset (the mean position of the sample)
    off = reg.integer_shifts - shifts.astype(np.int32)
    assert np.abs(off).max() <= 1 and np.all(off.max(axis=0) - off.min(axis=0) <= 1) and reg.template.shape == (d1, d2)
    assert np.all(np.isfinite(reg.template)) and reg.template.std() > 10
    none = localmd_amd.register_movie(mov, max_shift=ms, template_frames=50, template_iters=0, ctx=gpu_ctx)
    assert np.allclose(none.template, mov[sample].mean(axis=0), rtol=1e-5)
    src = _Counting(mov)
    localmd_amd.apply_shifts(src, dev, shifts, frame_batch_size=1024, ctx=gpu_ctx)
    assert np.all(src.count == 1)
    # a source that fails midway: the file this call created is gone
    for suffix in (".npy", ".tif"):
        p = tmp_path / ("bad" + suffix)
        with pytest.raises(OSError):
            localmd_amd.register_movie(_Counting(mov, fail_after=1500), str(p), max_shift=ms, template=base,
                                       frame_batch_size=1024, ctx=gpu_ctx)
        assert not p.exists()


def test_device_tensors_of_other_dtypes_and_aliased_destinations(gpu_ctx):
    """A device tensor whose dtype the kernels do not read is staged as fp32, the template's sample included: the bits
    of its fp32 copy.  A destination that shares storage with the movie is refused before any work."""
    import torch

    mov, _, _ = planted("small")
    ms = PLANTED["small"]["max_shift"]
    whole = np.rint(mov).astype(np.float32)                      # exact in float16, int32 and float64
    kw = dict(max_shift=ms, template_frames=20, ctx=gpu_ctx)
    want_out = torch.empty(whole.shape, dtype=torch.float32, device=gpu_ctx.device)
    want = localmd_amd.register_movie(torch.from_numpy(whole).to(gpu_ctx.device), want_out, **kw)
    assert np.any(want.shifts != 0)
    for dt in (torch.float64, torch.float16, torch.int32):
        src = torch.from_numpy(whole).to(gpu_ctx.device).to(dt)
        out = torch.empty(whole.shape, dtype=torch.float32, device=gpu_ctx.device)
        reg = localmd_amd.register_movie(src, out, **kw)
        assert reg.template.tobytes() == want.template.tobytes(), dt
        assert reg.shifts.tobytes() == want.shifts.tobytes() and reg.peak.tobytes() == want.peak.tobytes(), dt
        assert bool((out == want_out).all()), dt
    dev = torch.from_numpy(whole).to(gpu_ctx.device)
    before = dev.clone()
    for out in (dev, dev[:], dev.view(-1)[: dev.numel()].view(dev.shape)):
        with pytest.raises(ValueError, match="shares memory"):
            localmd_amd.register_movie(dev, out, **kw)
        with pytest.raises(ValueError, match="shares memory"):
            localmd_amd.apply_shifts(dev, out, np.ones((len(whole), 2)), ctx=gpu_ctx)
    big = torch.zeros((len(whole) + 3,) + whole.shape[1:], dtype=torch.float32, device=gpu_ctx.device)
    with pytest.raises(ValueError, match="shares memory"):       # aliased at a frame offset
        localmd_amd.register_movie(big[:len(whole)], big[3:], **kw)
    assert bool((dev == before).all())


def test_device_memory_does_not_grow_with_the_movie(gpu_ctx):
    import torch

    mov, base, _ = planted("stream")
    ms = PLANTED["stream"]["max_shift"]
    peaks = {}
    for n in (2048, 8192):
        m = np.concatenate([mov] * 4)[:n]
        out = np.empty(m.shape, np.float32)
        gpu_ctx.sync()
        gc.collect()                                   # device tensors that earlier tests left in reference cycles would be
        torch.cuda.empty_cache()                       # freed during the first call and lower its peak
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        localmd_amd.register_movie(m, out, max_shift=ms, template=base, frame_batch_size=1024, ctx=gpu_ctx)
        peaks[n] = torch.cuda.max_memory_allocated() - start
    D = mov.shape[1] * mov.shape[2]
    plan = RG.register_device_bytes(d1=mov.shape[1], d2=mov.shape[2], nb=1024, esize=4, host_source=True, n_batches=2,
                                    my=ms[0], mx=ms[1], out_esize=4, host_dest=True)
    assert peaks[8192] <= peaks[2048] + 4096, peaks
    assert 2 * 1024 * D * 4 <= peaks[2048] <= plan, (peaks, plan)


def test_registration_gives_the_decomposition_its_rank_back(gpu_ctx):
    """The point of the feature: the shifted movie needs more components than the still one; registered and cropped to
    ``valid`` it needs no more than the still one.  The planted motion and gains wander on a time scale of 40 frames:
    motion drawn afresh for every frame is white in time, which the decomposition discards like any other noise."""
    import torch

    mov, base, shifts = planted("e2e")
    ms = PLANTED["e2e"]["max_shift"]
    still, _, _ = R.planted_movie(moving=False, **PLANTED["e2e"])
    T, d1, d2 = mov.shape
    out = torch.empty((T, d1, d2), dtype=torch.float32, device=gpu_ctx.device)
    reg = localmd_amd.register_movie(mov, out, max_shift=ms, template=base, subpixel=False, ctx=gpu_ctx)
    assert np.array_equal(reg.shifts, shifts)
    y0, y1, x0, x1 = reg.valid
    assert (y1 - y0, x1 - x0) == (40, 40)

    def rank(x):
        np.random.seed(1)
        pmd, diag = localmd_amd.localmd_decomposition(x, (20, 20), T, max_components=12, background_rank=2, seed=9,
                                                      sim_iters=10, return_diagnostics=True, ctx=gpu_ctx)
        return int(np.sum(diag["tile_ranks"]))

    r_reg = rank(out[:, y0:y1, x0:x1].contiguous())
    r_still = rank(np.ascontiguousarray(still[:, y0:y1, x0:x1]))
    r_moved = rank(np.ascontiguousarray(mov[:, y0:y1, x0:x1]))
    print("total rank: registered", r_reg, "still", r_still, "shifted", r_moved)
    assert r_reg <= r_still < r_moved
