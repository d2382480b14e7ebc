"""Host side of the spatial filter (localmd_amd.spatial): the float32 emulation against float64, the border rule, the
weights, exact cases, argument checks and the memory plan; and the admissibility of the planted one-photon movies that
tests/test_gpu_register_prefilter.py registers (in float64, so that what the GPU test asserts is a property of the
method and not of the kernels)."""
import inspect

import numpy as np
import pytest

import localmd_amd
from localmd_amd import piecewise as PW
from localmd_amd import register as RG
from localmd_amd import spatial as S
from tests import register_ref as R
from tests import spatial_ref as SR


def test_names_are_exported():
    for name in ("SpatialFilter", "spatial_filter", "filter_frames", "filter_movie"):
        assert name in localmd_amd.__all__ and hasattr(localmd_amd, name)
    for f in (localmd_amd.register_movie, localmd_amd.register_piecewise):
        assert inspect.signature(f).parameters["prefilter"].default is None


def test_reflect_is_numpys_symmetric_padding():
    for d in (1, 2, 5, 33):
        for r in range(0, min(d, 32) + 1):
            want = np.pad(np.arange(d), r, mode="symmetric")
            assert np.array_equal(S.reflect_index(np.arange(-r, d + r), d), want), (d, r)
            assert [SR.refl(i, d) for i in range(-r, d + r)] == want.tolist()


_CASES = [  # (kind, sigma, radius, d1, d2)
    ("bandpass", 1.5, None, 31, 63), ("lowpass", 1.5, None, 33, 65), ("highpass", 1.5, None, 33, 65),
    ("bandpass", (0.8, 3.0), None, 20, 40), ("lowpass", (2.0, 1.0), (7, 1), 19, 12), ("highpass", (1.0, 4.0), (0, 9), 9, 21),
    ("bandpass", 2.0, 0, 8, 8), ("bandpass", 1.0, (0, 3), 1, 9), ("lowpass", 3.0, (5, 7), 5, 7), ("bandpass", 9.0, 32, 32, 40),
    ("highpass", 2.0, (1, 1), 1, 1),
]


@pytest.mark.parametrize("case", _CASES, ids=lambda c: "{}-{}-{}-{}x{}".format(*c))
def test_emulation_against_float64_within_the_bound(case):
    kind, sigma, radius, d1, d2 = case
    filt = S.spatial_filter(sigma, kind, radius)
    rng = np.random.default_rng(3)
    frames = (rng.standard_normal((3, d1, d2)) * 500 + 1000).astype(np.float32)
    got = S.filter_frames(frames, filt)
    assert got.dtype == np.float32 and got.shape == frames.shape
    err, bound = np.abs(got - SR.filter64(frames, filt)), SR.forward_bound(frames, filt)
    assert np.all(err <= bound), (err / bound).max()
    # one frame alone, a (d1, d2) image and an integer source give the same bits
    assert R.same_bits(S.filter_frames(frames[1], filt), got[1])
    u16 = np.rint(np.abs(frames)).astype(np.uint16)
    assert R.same_bits(S.filter_frames(u16, filt), S.filter_frames(u16.astype(np.float32), filt))


def test_weights_and_fields():
    f = S.spatial_filter(1.5)
    assert (f.kind, f.sigma, f.ry, f.rx, f.centre) == ("bandpass", (1.5, 1.5), 3, 3, 0.0)
    assert f.wy.dtype == np.float32 and f.wy.shape == (7,) and np.array_equal(f.wy, f.wx)
    g = np.exp(-np.arange(-3, 4) ** 2 / (2 * 1.5 ** 2))
    assert np.array_equal(f.wy, (g / g.sum()).astype(np.float32))
    assert f.box == float(np.float32(1 / 49))
    f = S.spatial_filter((0.6, 7.0), "lowpass")
    assert (f.ry, f.rx, f.centre, f.box, f.sigma) == (2, 14, 0.0, 0.0, (0.6, 7.0))
    f = S.spatial_filter(2.0, "highpass", (1, 4))
    assert (f.ry, f.rx, f.centre, f.box) == (1, 4, 1.0, 0.0) and np.all(f.wy < 0) and np.all(f.wx > 0)
    assert abs(float(f.wx.astype(np.float64).sum()) - 1) < 9 * SR.U and abs(float(f.wy.astype(np.float64).sum()) + 1) < 3 * SR.U
    f = S.spatial_filter(1.0, radius=0)
    assert f.wy.tolist() == [1.0] and f.box == 1.0
    own = S.SpatialFilter([0.25, 0.5, 0.25], [1.0], centre=2, box=0.5)
    assert (own.ry, own.rx, own.centre, own.box, own.kind, own.sigma) == (1, 0, 2.0, 0.5, None, None)
    assert S.as_filter(own) is own and S.as_filter(2.0).kind == "bandpass"


def test_bandpass_sums_to_zero_and_removes_a_constant():
    for sigma, radius in ((1.5, None), ((0.7, 5.0), None), (4.0, (3, 20)), (16.0, 32)):
        f = S.spatial_filter(sigma, "bandpass", radius)
        n = (2 * f.ry + 1) * (2 * f.rx + 1)
        total = float(np.outer(f.wy.astype(np.float64), f.wx.astype(np.float64)).sum()) - f.box * n
        assert abs(total) <= (2 * f.ry + 2 * f.rx + 3) * SR.U, total     # each weight and box rounded once
        img = np.full((1, 40, 70), 1234.5, np.float32)
        out = S.filter_frames(img, f)
        assert np.all(np.abs(out - SR.filter64(img, f)) <= SR.forward_bound(img, f))
        assert np.all(np.abs(out) <= SR.forward_bound(img, f) + abs(total) * 1234.5)
        assert np.abs(out).max() < 1234.5 * 1e-4


def test_dyadic_weights_on_small_integers_are_exact():
    rng = np.random.default_rng(5)
    img = rng.integers(-200, 200, (2, 13, 17))
    w = np.array([0.25, 0.5, 0.25], np.float32)
    for centre, box in ((0.0, 0.0), (2.0, 0.0), (0.0, 0.125), (-1.0, 0.5)):
        f = S.SpatialFilter(w, w, centre, box)
        p = np.pad(img, ((0, 0), (1, 1), (1, 1)), mode="symmetric").astype(np.int64)
        k = np.array([1, 2, 1], np.int64)
        acc = np.zeros(img.shape, np.int64)
        tot = np.zeros(img.shape, np.int64)
        for i in range(3):
            for j in range(3):
                acc += k[i] * k[j] * p[:, i:i + 13, j:j + 17]
                tot += p[:, i:i + 13, j:j + 17]
        want = centre * img + acc / 16.0 - box * tot                     # multiples of 1 / 16 below 2^12: exact
        for dt in (np.float32, np.int16):
            got = S.filter_frames(img.astype(dt), f)
            assert np.array_equal(got.astype(np.float64), want), (centre, box, dt)
        assert np.array_equal(S.filter_frames(img.astype(np.float32), f, "int16"),
                              np.clip(np.rint(want), -32768, 32767).astype(np.int16))
        assert np.array_equal(S.filter_frames(img.astype(np.float32), f, "uint16"),
                              np.clip(np.rint(want), 0, 65535).astype(np.uint16))


def test_nan_and_inf_spread_exactly_over_the_window():
    rng = np.random.default_rng(6)
    base = rng.standard_normal((1, 40, 60)).astype(np.float32)
    spots = {(10, 12): np.nan, (10, 45): np.inf, (29, 30): -np.inf}
    img = base.copy()
    for (y, x), v in spots.items():
        img[0, y, x] = v
    for kind, radius in (("lowpass", (2, 5)), ("bandpass", (3, 4)), ("highpass", (4, 0))):
        f = S.spatial_filter(2.0, kind, radius)
        out = S.filter_frames(img, f)[0]
        hit = np.zeros((40, 60), bool)
        for (y, x), v in spots.items():
            win = (slice(y - f.ry, y + f.ry + 1), slice(x - f.rx, x + f.rx + 1))
            hit[win] = True
            if kind == "lowpass":
                assert np.all(np.isnan(out[win])) if np.isnan(v) else np.all(out[win] == v), (kind, v)
            else:
                assert not np.isfinite(out[win]).any()
        assert np.array_equal(~np.isfinite(out), hit), kind
        assert R.same_bits(out[~hit], S.filter_frames(base, f)[0][~hit])
    assert S.filter_frames(img, S.spatial_filter(2.0, "lowpass", (2, 5)), "uint16")[0, 10, 12] == 0        # NaN -> 0
    assert S.filter_frames(img, S.spatial_filter(2.0, "lowpass", (2, 5)), "int16")[0, 29, 30] == -32768


def test_argument_checks():
    for bad in (0, -1.0, np.nan, np.inf, "2", (1.0,), (1.0, 2.0, 3.0), (1.0, 0.0), True, None):
        with pytest.raises(ValueError, match="sigma"):
            S.spatial_filter(bad)
    with pytest.raises(ValueError, match="kind"):
        S.spatial_filter(1.0, "notch")
    for bad in (-1, 1.5, (1,), (1, -2), True):
        with pytest.raises(ValueError, match="radius"):
            S.spatial_filter(1.0, radius=bad)
    with pytest.raises(ValueError, match="larger than 32"):
        S.spatial_filter(17.0)
    with pytest.raises(ValueError, match="larger than 32"):
        S.spatial_filter(1.0, radius=(33, 1))
    assert S.spatial_filter(16.0).ry == 32
    with pytest.raises(ValueError, match="2 r \\+ 1"):
        S.SpatialFilter([0.5, 0.5], [1.0])
    with pytest.raises(ValueError, match="2 r \\+ 1"):
        S.SpatialFilter(np.ones(67), [1.0])
    img = np.zeros((2, 6, 9), np.float32)
    with pytest.raises(ValueError, match="radii"):
        S.filter_frames(img, S.spatial_filter(1.0, radius=(7, 1)))
    with pytest.raises(ValueError, match="radii"):
        S.filter_frames(img, S.spatial_filter(1.0, radius=(1, 10)))
    assert S.filter_frames(img, S.spatial_filter(1.0, radius=(6, 9))).shape == img.shape
    with pytest.raises(ValueError, match="dtype"):
        S.filter_frames(img, 1.0, dtype="float64")
    with pytest.raises(ValueError, match="shape"):
        S.filter_frames(np.zeros(5, np.float32), 1.0)
    # the front doors refuse before any device work: these hold on a machine without a device
    mov = np.zeros((4, 6, 9), np.float32)
    out = np.zeros((4, 6, 9), np.float32)
    for kw, exc, match in ((dict(filt_or_sigma=-1.0), ValueError, "sigma"), (dict(filt_or_sigma=1.0, kind="x"), ValueError, "kind"),
                           (dict(filt_or_sigma=4.0), ValueError, "radii"), (dict(filt_or_sigma=1.0, dtype="int8"), ValueError, "dtype"),
                           (dict(filt_or_sigma=1.0, frame_batch_size=0), ValueError, "frame_batch_size"),
                           (dict(filt_or_sigma=1.0, bigtiff=1), ValueError, "bigtiff")):
        with pytest.raises(exc, match=match):
            localmd_amd.filter_movie(mov, out, **kw)
    with pytest.raises(TypeError, match="destination"):
        localmd_amd.filter_movie(mov, None, 1.0)
    with pytest.raises(ValueError, match="shares memory"):
        localmd_amd.filter_movie(mov, mov, 1.0)
    with pytest.raises(ValueError, match="no frames"):
        localmd_amd.filter_movie(mov[:0], out[:0], 1.0)
    with pytest.raises(ValueError, match="shape"):
        localmd_amd.filter_movie(mov[0], out, 1.0)
    big = np.zeros((4, 40, 40), np.float32)
    for f in (localmd_amd.register_movie, localmd_amd.register_piecewise):
        kw = dict(max_shift=2, patch=16, stride=12) if f is localmd_amd.register_piecewise else dict(max_shift=2)
        with pytest.raises(ValueError, match="sigma"):
            f(big, prefilter=-2.0, **kw)
        with pytest.raises(ValueError, match="sigma"):
            f(big, prefilter="band", **kw)
        with pytest.raises(ValueError, match="larger than 32"):
            f(big, prefilter=40.0, **kw)
        with pytest.raises(ValueError, match="radii"):
            f(big[:, :, :30], prefilter=S.spatial_filter(9.0, radius=(1, 32)), **kw)


def test_memory_plans():
    D = 64 * 96
    base = dict(d1=64, d2=96, esize=2, host_source=True)
    one = S.filter_device_bytes(nb=1000, n_batches=1, **base)
    assert one == 1000 * D * 2 + (1 << 20)
    two = S.filter_device_bytes(nb=2048, n_batches=3, out_esize=4, host_dest=True, **base)
    assert two == 2 * 2048 * D * 2 + 2 * 1024 * D * 4 + (1 << 20)
    assert S.filter_device_bytes(nb=2048, n_batches=3, d1=64, d2=96, esize=4, host_source=False) == 2048 * D * 4 + (1 << 20)
    # the registration bounds: the prefilter adds the block scratch, the filtered sample and the template's two images
    kw = dict(d1=64, d2=96, nb=2048, esize=2, host_source=True, n_batches=2, my=4, mx=5, n_sample=200, out_esize=4,
              host_dest=True)
    plain = RG.register_device_bytes(**kw)
    assert RG.register_device_bytes(prefilter=False, **kw) == plain
    assert RG.register_device_bytes(prefilter=True, **kw) == plain + 4 * 1024 * D + 4 * 200 * D + 8 * D
    kw.pop("my"), kw.pop("mx")
    assert RG.register_device_bytes(prefilter=True, **kw) == RG.register_device_bytes(**kw)       # apply_shifts: no estimate
    pg = PW.PatchGrid(64, 96, (4, 5), 2, 24, 16)
    kw.update(gy=pg.gy, gx=pg.gx, pg=pg)
    plain = PW.piecewise_device_bytes(**kw)
    assert PW.piecewise_device_bytes(prefilter=True, **kw) == plain + 4 * 1024 * D + 4 * 200 * D + 8 * D


def test_registration_objects_carry_the_prefilter():
    f = S.spatial_filter(1.5)
    z = np.zeros((3, 2))
    reg = RG.Registration(z, z, np.zeros(3), np.zeros((20, 20), np.float32), (2, 2))
    assert reg.prefilter is None
    reg = RG.Registration(z, z, np.zeros(3), np.zeros((20, 20), np.float32), (2, 2), prefilter=f)
    assert reg.prefilter is f
    assert RG.check_prefilter(None, 20, 20) is None and RG.check_prefilter(f, 20, 20) is f
    got = RG.check_prefilter((1.0, 2.0), 20, 20)
    assert (got.kind, got.sigma, got.ry, got.rx) == ("bandpass", (1.0, 2.0), 2, 4)


# ---- the planted one-photon movies, in float64 ----------------------------------------------------------------------
def test_explicit_template_case_is_admissible():
    """Without a filter the correlation follows the static hill; with it every shift is right and the peak stands out by
    far more than the fp32 pipeline can move a surface entry."""
    mov, tmpl, shifts = SR.one_photon("explicit")
    ms = SR.ONE_PHOTON["explicit"]["max_shift"]
    filt = S.spatial_filter(SR.SIGMA)
    ints, _ = SR.match64(mov, tmpl, ms)
    wrong = int((ints != shifts).any(axis=1).sum())
    print("unfiltered: wrong", wrong, "of", len(mov))
    assert wrong >= 20
    ints, surf = SR.match64(SR.filter64(mov, filt), SR.filter64(tmpl, filt).astype(np.float32), ms)
    assert np.array_equal(ints, shifts)
    worst = min(SR.peak_gap(s) / (2 * SR.propagated_bound(f, tmpl, filt, ms).max()) for f, s in zip(mov, surf))
    rel = min(SR.peak_gap(s) / np.abs(s).max() for s in surf)
    print("peak gap / (2 x bound): worst", worst, "smallest relative gap", rel)
    assert worst > 1 and rel > 0.1
    # the emulated fp32 frames give the same peaks (what the device matches)
    ints32, _ = SR.match64(S.filter_frames(mov, filt), S.filter_frames(tmpl, filt), ms)
    assert np.array_equal(ints32, shifts)


def test_built_template_case_is_admissible():
    """The template built through the filter (two iterations, all 40 frames) recovers every planted shift with no common
    offset; built without the filter it recovers next to none."""
    mov, _, shifts = SR.one_photon("built")
    ms = SR.ONE_PHOTON["built"]["max_shift"]
    filt = S.spatial_filter(SR.SIGMA)
    built = SR.build_template64(mov, filt, ms, 2)
    ints, _ = SR.match64(SR.filter64(mov, filt), SR.filter64(built, filt).astype(np.float32), ms)
    assert np.array_equal(ints, shifts)
    plain = SR.build_template64(mov, None, ms, 2)
    ints, _ = SR.match64(mov, plain.astype(np.float32), ms)
    assert int((ints != shifts).any(axis=1).sum()) >= 30
