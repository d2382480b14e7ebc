"""The host side of piecewise registration (localmd_amd.piecewise) against the NumPy / SciPy statements of
tests/piecewise_ref.py: the patch geometry, the field tables and the fp32 field, warp_frames, the fallback rules, the
argument checks and the memory plan, WarpedMovie, and what the float64 reference achieves on the planted movie.  No GPU."""
import numpy as np
import pytest
from scipy import ndimage

import localmd_amd
from localmd_amd import piecewise as PW
from localmd_amd import register as RG
from tests import piecewise_ref as Q
from tests import register_ref as R
from tests.piecewise_planted import FIELD_RMS_PIECEWISE, FIELD_RMS_RIGID, PLANTED, planted, reference, settings

U = 2.0 ** -24


def test_exports():
    for name in ("register_piecewise", "PiecewiseRegistration", "apply_field", "warp_frames", "WarpedMovie"):
        assert name in localmd_amd.__all__ and hasattr(localmd_amd, name)


# ---- geometry --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d1,patch,stride,want", [
    (16 + 32, 32, 24, [0]),                 # Hh == ph: one patch
    (16 + 33, 32, 24, [0, 1]),              # one pixel more: a second patch, pulled back to the end of the area
    (16 + 80, 32, 24, [0, 24, 48]),         # the stride divides Hh - ph
    (16 + 90, 32, 24, [0, 24, 48, 58]),     # the last patch is pulled back
    (16 + 40, 8, 8, [0, 8, 16, 24, 32]),
    (16 + 12, 8, 1, [0, 1, 2, 3, 4]),
])
def test_starts_and_centres(d1, patch, stride, want):
    pg = PW.PatchGrid(d1, 70, (5, 4), (3, 2), (patch, 16), (stride, 16))
    assert pg.starts[0].tolist() == want == Q.starts(d1 - 16, patch, stride)
    assert (pg.oy, pg.ox, pg.Hh, pg.Ww) == (8, 6, d1 - 16, 58) and pg.gy == len(want) and pg.P == pg.gy * pg.gx
    geo = Q.geometry(d1, 70, (5, 4), (3, 2), (patch, 16), (16 if stride > 16 else stride, 16))
    assert np.array_equal(pg.centers[0], 8 + np.array(want) + (patch - 1) / 2)
    assert np.array_equal(pg.centers[1], geo["xc"]) and pg.starts[1].tolist() == geo["xstart"]
    assert pg.starts[1][-1] == 58 - 16 and np.all(np.diff(pg.starts[1]) <= 16)      # the area is covered without gaps


def test_tables_against_interp_and_constant_outside():
    rng = np.random.default_rng(0)
    for d, centres in ((60, [10.5, 30.5, 41.5]), (40, [19.5]), (50, [7.0, 8.0]), (33, [3.5, 11.5, 19.5, 27.5, 29.5])):
        idx, w = PW.field_tables(centres, d)
        ridx, rw = Q.axis_table(centres, d)
        assert np.array_equal(idx, ridx) and w.tobytes() == rw.tobytes() and idx.dtype == np.int32 and w.dtype == np.float32
        assert idx.min() >= 0 and idx.max() <= max(len(centres) - 2, 0)
        vals = rng.standard_normal(len(centres))
        y = np.arange(d, dtype=np.float64)
        if len(centres) == 1:
            assert not idx.any() and not w.any()
            continue
        got = vals[idx] + w.astype(np.float64) * (vals[idx + 1] - vals[idx])
        assert np.abs(got - np.interp(y, centres, vals)).max() <= 4 * U * np.abs(vals).max()
        assert np.all(got[y <= centres[0]] == vals[0]) and np.all(w[y >= centres[-1]] == 1) and np.all(w[y <= centres[0]] == 0)
    with pytest.raises(ValueError):
        PW.field_tables([5.0, 5.0], 10)


def test_field_against_float64_and_uniform_grid_exact():
    """The fp32 field against the float64 bilinear interpolation.  With M = max |g|: a lerp l = g0 + w (g1 - g0) has a
    rounded weight (relative u, on a difference of at most 2 M), a rounded difference (u 2 M), a rounded product (u 2 M)
    and a rounded sum (u 3 M at most): 9 u M to first order.  The second lerp inherits 9 u M from top, 18 u M through
    (bot - top), and adds the same four roundings on values of at most 3 M: below 40 u M in all."""
    rng = np.random.default_rng(1)
    d1, d2 = 75, 90
    for gy, gx in ((1, 1), (1, 3), (2, 2), (3, 5), (5, 1)):
        yc = np.sort(rng.choice(np.arange(5, d1 - 5), gy, replace=False)) + 0.5
        xc = np.sort(rng.choice(np.arange(5, d2 - 5), gx, replace=False)) + 0.5
        tabs = PW.make_tables((yc, xc), d1, d2)
        grid = (rng.standard_normal((gy, gx, 2)) * 3).astype(np.float32)
        got = PW.lerp_field(grid, tabs)
        assert got.dtype == np.float32 and got.tobytes() == Q.field32(grid, tabs).tobytes()
        want = Q.field64(grid, yc, xc, d1, d2)
        assert np.abs(got - want).max() <= 40 * U * np.abs(grid).max(), (gy, gx)
        flat = np.empty((gy, gx, 2), np.float32)
        flat[..., 0], flat[..., 1] = np.float32(1.3), np.float32(-2.7)
        f = PW.lerp_field(flat, tabs)
        assert np.all(f[..., 0] == np.float32(1.3)) and np.all(f[..., 1] == np.float32(-2.7))


# ---- warp_frames -----------------------------------------------------------------------------------------------------
def _frames(rng, src, shape):
    if src == "float32":
        return (300.0 + 80.0 * rng.standard_normal(shape)).astype(np.float32)
    info = np.iinfo(src)
    return rng.integers(info.min, info.max + 1, shape).astype(src)


@pytest.mark.parametrize("dst", ["float32", "uint16", "int16"])
@pytest.mark.parametrize("border", ["nearest", 123.0])
def test_warp_uniform_integer_grid_equals_shift_frames(dst, border):
    rng = np.random.default_rng(2)
    pg = PW.PatchGrid(40, 56, (4, 4), (2, 2), (12, 16), (8, 12))
    tabs = PW.make_tables(pg.centers, 40, 56)
    shifts = np.array([(0, 0), (2, -3), (-4, 1), (6, 6), (-45, 3), (3, 70)], dtype=np.float64)
    for src in ("float32", "uint16", "int16"):
        frames = _frames(rng, src, (len(shifts), 40, 56))
        grid = np.broadcast_to(shifts[:, None, None, :], (len(shifts), pg.gy, pg.gx, 2))
        got = PW.warp_frames(frames, grid, tabs, border, dst)
        assert got.tobytes() == RG.shift_frames(frames, shifts, border, dst).tobytes(), src
        assert got.tobytes() == Q.warp_movie(frames, grid, Q.tables(Q.geometry(40, 56, (4, 4), (2, 2), (12, 16), (8, 12))),
                                             border, dst).tobytes()


def _bilinear64(frame, field, fill=None):
    """The float64 bilinear sample at (y + s_y, x + s_x): nearest edge pixel outside the frame, or ``fill``."""
    d1, d2 = frame.shape
    f = np.asarray(frame, dtype=np.float64)
    y = np.clip(np.arange(d1)[:, None] + field[..., 0], -1, d1)
    x = np.clip(np.arange(d2)[None, :] + field[..., 1], -1, d2)
    y0, x0 = np.floor(y).astype(int), np.floor(x).astype(int)
    fy, fx = y - y0, x - x0

    def g(yy, xx):
        v = f[np.clip(yy, 0, d1 - 1), np.clip(xx, 0, d2 - 1)]
        return v if fill is None else np.where((yy >= 0) & (yy < d1) & (xx >= 0) & (xx < d2), v, fill)

    return ((1 - fy) * (1 - fx) * g(y0, x0) + (1 - fy) * fx * g(y0, x0 + 1) + fy * (1 - fx) * g(y0 + 1, x0)
            + fy * fx * g(y0 + 1, x0 + 1))


def test_warp_fractional_fields_against_float64():
    """warp_frames against float64 bilinear sampling at the fp32 field's own positions.  The coordinate fl(y + s) is off
    by at most delta = u (d + max |s| + 1); bilinear interpolation is continuous with slope at most 2 V per axis
    (V = max |pixel|), so that costs 4 delta V; the four weights (three roundings each), the products and the three sums
    cost below 12 u V."""
    rng = np.random.default_rng(3)
    d1, d2 = 48, 64
    pg = PW.PatchGrid(d1, d2, (4, 4), (3, 3), (12, 16), (9, 12))
    tabs = PW.make_tables(pg.centers, d1, d2)
    frames = _frames(rng, "float32", (4, d1, d2))
    grid = (rng.standard_normal((4, pg.gy, pg.gx, 2)) * 2.5).astype(np.float32)
    grid[3] *= 20                                                     # far beyond the frame
    V = float(np.abs(frames).max())
    for border in ("nearest", -50.0):
        got = PW.warp_frames(frames, grid, tabs, border)
        for k in range(4):
            field = PW.lerp_field(grid[k], tabs).astype(np.float64)
            crossing = np.unique(np.floor(np.arange(d1)[:, None] + field[..., 0]) - np.arange(d1)[:, None])
            assert len(crossing) > 1                                  # the field crosses integer boundaries inside the frame
            want = _bilinear64(frames[k], field, None if border == "nearest" else border)
            delta = U * (max(d1, d2) + np.abs(field).max() + 1)
            assert np.abs(got[k] - want).max() <= (4 * delta + 12 * U) * max(V, 50.0), (border, k)
            if border == "nearest":
                assert np.abs(Q.warp64(frames[k], field) - want).max() <= 1e-9 * V       # scipy.ndimage.map_coordinates
        assert R.same_bits(got, Q.warp_movie(frames, grid, Q.tables(Q.geometry(d1, d2, (4, 4), (3, 3), (12, 16), (9, 12))),
                                             border))
        for dst in ("uint16", "int16"):
            q = PW.warp_frames(frames, grid, tabs, border, dst)
            assert q.dtype == np.dtype(dst) and np.array_equal(q, R.quantize(got, dst))
    for src in ("uint16", "int16"):
        fr = _frames(rng, src, (4, d1, d2))
        assert np.array_equal(PW.warp_frames(fr, grid, tabs), PW.warp_frames(fr.astype(np.float32), grid, tabs))


def test_warp_nan_and_huge_fields_stay_in_range():
    rng = np.random.default_rng(4)
    d1, d2 = 20, 30
    tabs = PW.make_tables(([5.5, 14.5], [6.5, 15.5, 24.5]), d1, d2)
    frames = _frames(rng, "float32", (3, d1, d2))
    grid = np.zeros((3, 2, 3, 2), np.float32)
    grid[0, 0, 0], grid[1], grid[2, 1, 2] = np.nan, 3e38, (-np.inf, 1e30)
    got = PW.warp_frames(frames, grid, tabs, 7.0)
    assert R.same_bits(got, Q.warp_movie(frames, grid, tabs, 7.0))
    assert np.all(got[1] == 7.0) and np.all(got[0, 0, 0] == 7.0)      # NaN acts as -1: outside, the fill


# ---- the host finish ---------------------------------------------------------------------------------------------------
def test_fallback_rules_at_limit_and_valid():
    rng = np.random.default_rng(5)
    d1, d2 = 60, 70
    pg = PW.PatchGrid(d1, d2, (4, 4), (2, 2), (16, 16), (12, 12))
    template = (300 + 80 * rng.standard_normal((d1, d2))).astype(np.float32)
    a, b = pg.oy + pg.starts[0][1], pg.ox + pg.starts[1][2]
    template[a:a + 16, b:b + 16] = 250.0                                 # a constant patch: t' = 0
    tps, zero = PW.patch_templates(template, pg)
    assert zero.sum() == 1 and zero[1, 2] and tps.tobytes() == Q.packed_templates(
        template, Q.geometry(d1, d2, (4, 4), (2, 2), (16, 16), (12, 12))).tobytes()
    m = 5
    surf = rng.standard_normal((m, pg.gy, pg.gx, 5, 5)).astype(np.float32)
    surf[0, 0, 0] = np.nan                                               # no finite entry
    surf[1, 0, 1] = -np.inf
    surf[2, 1, 1, 0, 3] = 99.0                                           # a peak on the edge of the deviation range
    surf[:, 1, 2] = 0.0                                                  # what the zero patch gives
    centre = rng.integers(-4, 5, (m, 2)).astype(np.int32)
    rigid = centre + rng.uniform(-0.5, 0.5, (m, 2))
    parg, ppk, pnb = np.zeros((m, pg.gy, pg.gx, 2), np.int32), np.zeros((m, pg.gy, pg.gx), np.float32), \
        np.zeros((m, pg.gy, pg.gx, 3, 3), np.float32)
    for k in range(m):
        for i in range(pg.gy):
            for j in range(pg.gx):
                parg[k, i, j], ppk[k, i, j], pnb[k, i, j] = R.peak(surf[k, i, j])
    for subpixel in (True, False):
        sh, ints, fb = PW.finish_patches(rigid, centre, parg, ppk, pnb, zero, subpixel)
        for k in range(m):
            rsh, rints, rpk, rfb = Q.finish_frame(surf[k], tps, centre[k], rigid[k], subpixel)
            assert np.array_equal(sh[k], rsh) and np.array_equal(ints[k], rints) and np.array_equal(fb[k], rfb), (k, subpixel)
        assert fb[0, 0, 0] and fb[1, 0, 1] and fb[:, 1, 2].all() and fb.sum() == 2 + m
        assert np.array_equal(sh[0, 0, 0], rigid[0]) and np.array_equal(ints[3, 1, 2], centre[3])
    sh, ints, fb = PW.finish_patches(rigid, centre, parg, ppk, pnb, zero, True)
    rig = RG.Registration(rigid, centre, np.ones(m, np.float32), template, (4, 4))
    reg = PW.PiecewiseRegistration(rig, sh, ints, ppk, fb, pg, template)
    dev = np.abs(ints - centre[:, None, None, :]).max(axis=-1)
    want = {tuple(t) for t in np.argwhere((dev == 2) & ~fb)}
    assert (2, 1, 1) in want and {tuple(t) for t in reg.at_limit} == want
    assert not any(fb[tuple(t)] for t in reg.at_limit)
    assert reg.valid == RG.valid_rect(sh.reshape(-1, 2), d1, d2) and reg.shifts.shape == (m, pg.gy, pg.gx, 2)
    f = reg.field(2)
    assert f.shape == (d1, d2, 2) and f.dtype == np.float32
    assert f.tobytes() == Q.field32(sh[2].astype(np.float32), Q.tables(Q.geometry(d1, d2, (4, 4), (2, 2), (16, 16),
                                                                                  (12, 12)))).tobytes()
    lo, hi = sh.min(axis=(0, 1, 2)), sh.max(axis=(0, 1, 2))             # a convex combination of the patch shifts
    assert np.all(f >= lo - 1e-5) and np.all(f <= hi + 1e-5)


# ---- arguments and the memory plan -------------------------------------------------------------------------------------
def test_argument_checks_come_before_device_work(tmp_path):
    mov = np.zeros((5, 64, 80), np.float32)
    bad = [dict(max_deviation=0), dict(max_deviation=8), dict(max_deviation=(3, 9)), dict(max_deviation=2.5),
           dict(patch=7), dict(patch=(64, 20)), dict(patch=(20, 200)), dict(stride=0), dict(stride=(25, 4), patch=24),
           dict(stride=(4, 25), patch=24), dict(max_shift=32), dict(max_shift=0), dict(max_shift=29), dict(patch="big"),
           dict(template=np.zeros((3, 3))), dict(template_frames=0), dict(template_iters=-1), dict(frame_batch_size=0),
           dict(border="wrap"), dict(dtype="float64"), dict(bigtiff=True), dict(patch=8, stride=1, max_shift=2,
                                                                             max_deviation=1)]
    for kw in bad:
        args = dict(max_shift=5, patch=24, stride=16)
        args.update(kw)
        with pytest.raises(ValueError):
            localmd_amd.register_piecewise(mov, **args)
    p = tmp_path / "never.npy"
    with pytest.raises(ValueError):
        localmd_amd.register_piecewise(mov, str(p), max_shift=5, patch=24, stride=30)
    assert not p.exists()
    with pytest.raises(ValueError, match="shares memory"):
        localmd_amd.register_piecewise(mov, mov, max_shift=5, patch=24, stride=16)
    with pytest.raises(ValueError):
        localmd_amd.register_piecewise(np.zeros((0, 64, 80), np.float32), max_shift=5, patch=24, stride=16)
    good = np.zeros((5, 3, 4, 2))
    cen = ([10.5, 30.5, 50.5], [10.5, 30.5, 50.5, 70.5])
    for shifts, centers in ((good, None), (good[:4], cen), (good[..., :1], cen), (good, (cen[0], cen[1][:3])),
                            (good, (cen[0][::-1], cen[1])), (good + np.nan, cen), (good + 2.0 ** 21, cen),
                            (np.zeros((5, 65, 4, 2)), cen)):
        with pytest.raises(ValueError):
            localmd_amd.apply_field(mov, np.empty_like(mov), shifts, centers=centers)
        with pytest.raises(ValueError):
            localmd_amd.WarpedMovie(mov, shifts, centers=centers)
    with pytest.raises(TypeError):
        localmd_amd.apply_field(mov, None, good, centers=cen)
    with pytest.raises(ValueError, match="shares memory"):
        localmd_amd.apply_field(mov, mov, good, centers=cen)


def test_memory_plan():
    pg = PW.PatchGrid(512, 512, 15, 3, 128, 96)
    assert (pg.gy, pg.gx, pg.P) == (5, 5, 25)
    kw = dict(d1=512, d2=512, esize=2, host_source=True, gy=5, gx=5, pg=pg, out_esize=4, host_dest=True)
    one = PW.piecewise_device_bytes(nb=1024, n_batches=3, **kw)
    assert one == PW.piecewise_device_bytes(nb=1024, n_batches=300, **kw)          # no term grows with the movie's length
    rigid = RG.register_device_bytes(d1=512, d2=512, nb=1024, esize=2, host_source=True, n_batches=3, my=15, mx=15,
                                     out_esize=4, host_dest=True)
    sub = PW.surface_frames(1024, pg)
    assert sub == 1024 and 4 * sub * 25 * 49 <= PW.SURFACE_CAP
    extra = one - rigid
    assert extra == (4 * 25 * 128 * 128 + PW.patch_workspace_bytes(sub, pg) + 4 * sub * 25 * 49 + 48 * 1024 * 25 + 40
                     + 8 * 1024 * 25 + 8 * 1024)
    assert PW.patch_workspace_bytes(1024, pg) == 1024 * 4 * 25 * 8 * 49 and PW.patch_workspace_bytes(10 ** 6, pg) <= 64 << 20
    many = PW.PatchGrid(512, 512, 15, 7, 16, 8)                                    # 3025 patches of 225 entries
    assert PW.surface_frames(1024, many) == (32 << 20) // (4 * many.P * 225) < 1024
    assert PW.piecewise_device_bytes(nb=1024, n_batches=2, d1=512, d2=512, esize=2, host_source=False, gy=5, gx=5) < rigid


# ---- WarpedMovie -----------------------------------------------------------------------------------------------------
def test_warped_movie_against_warp_frames():
    from localmd_amd.dataset import lazy_data_loader

    rng = np.random.default_rng(6)
    T, d1, d2 = 9, 40, 50
    pg = PW.PatchGrid(d1, d2, (3, 3), (2, 2), (12, 12), (10, 10))
    mov = _frames(rng, "uint16", (T, d1, d2))
    shifts = rng.standard_normal((T, pg.gy, pg.gx, 2)) * 2
    tabs = PW.make_tables(pg.centers, d1, d2)
    for border, dtype in (("nearest", None), (100.0, "uint16")):
        wm = localmd_amd.WarpedMovie(mov, shifts, border=border, dtype=dtype, centers=pg.centers)
        want = PW.warp_frames(mov, shifts, tabs, border, dtype)
        assert wm.shape == (T, d1, d2) and wm.dtype == want.dtype and isinstance(wm, lazy_data_loader)
        assert R.same_bits(wm[:], want) and R.same_bits(wm[[7, 2]], want[[7, 2]]) and R.same_bits(wm[3:5], want[3:5])
    rig = RG.Registration(np.zeros((T, 2)), np.zeros((T, 2)), np.ones(T), np.zeros((d1, d2)), (3, 3), 55.0)
    reg = PW.PiecewiseRegistration(rig, shifts, np.rint(shifts), np.ones((T, pg.gy, pg.gx)), np.zeros((T, pg.gy, pg.gx)),
                                   pg, np.zeros((d1, d2)), 55.0)
    assert R.same_bits(localmd_amd.WarpedMovie(mov, reg)[:], PW.warp_frames(mov, shifts, tabs, 55.0))


# ---- what the float64 reference achieves on the planted movie ---------------------------------------------------------
def test_reference_on_the_planted_movie():
    """Every integer peak of the reference, rigid and per patch, leads its runner-up by more than twice the kernel's
    forward bound, so a device whose surfaces are within the bound finds the same integers; and the recovered field is
    more than twice as close to the planted one as the rigid estimate."""
    mov, base, truth = planted("field")
    ref, kw = reference("field"), settings("field")
    geo = ref["geometry"]
    tps = Q.packed_templates(base, geo)
    tp = R.window_template(base, *kw["max_shift"])
    for k in range(len(mov)):
        c = ref["rigid"]["integer_shifts"][k]
        assert Q.peak_gap(ref["rigid"]["surfaces"][k]) > 2 * R.forward_bound(mov[k], tp, *kw["max_shift"]).max(), k
        for i in range(geo["gy"]):
            for j in range(geo["gx"]):
                bound = Q.forward_bound(mov[k], tps[i * geo["gx"] + j], geo, i, j, c).max()
                assert Q.peak_gap(ref["surfaces"][k, i, j]) > 2 * bound, (k, i, j)
    assert not ref["fallback"].any()
    tabs = Q.tables(geo)
    est = np.stack([Q.field32(g.astype(np.float32), tabs) for g in ref["shifts"]])
    valid = RG.valid_rect(ref["shifts"].reshape(-1, 2), *mov.shape[1:])
    rms = Q.field_rms(est, truth, valid)
    rigid = Q.field_rms(np.broadcast_to(ref["rigid"]["shifts"][:, None, None, :], truth.shape), truth, valid)
    print("field RMS inside valid: piecewise {:.4f} px, rigid {:.4f} px".format(rms, rigid))
    assert rms < 0.5 * rigid
    assert abs(rms - FIELD_RMS_PIECEWISE) < 0.01 and abs(rigid - FIELD_RMS_RIGID) < 0.01       # the values of DESIGN 4p
    assert np.abs(ref["integer_shifts"] - ref["rigid"]["integer_shifts"][:, None, None, :]).max() >= 1
    # the other planted movies of the GPU tests: the same room for their integers
    for name in ("rigid", "stream"):
        m2, b2, _ = planted(name)
        r2, k2 = reference(name), settings(name)
        g2 = r2["geometry"]
        t2 = Q.packed_templates(b2, g2)
        for k in range(0, len(m2), 7):
            c = r2["rigid"]["integer_shifts"][k]
            for i in range(g2["gy"]):
                for j in range(g2["gx"]):
                    bound = Q.forward_bound(m2[k], t2[i * g2["gx"] + j], g2, i, j, c).max()
                    assert Q.peak_gap(r2["surfaces"][k, i, j]) > 2 * bound, (name, k, i, j)
    assert PLANTED["field"]["movie"]["T"] == len(mov)
