"""Host side of the rolling baseline (localmd_amd.baseline) and the NumPy emulations the GPU tests compare with
(tests/baseline_ref.py): the sliding extrema against scipy.ndimage, the bin chains against float64 means, the bin centres
and the interpolation, the window -> h rule, argument checks, the Baseline checks, the memory plan, and the opening
property that makes "maximin" a baseline."""
import numpy as np
import pytest
import scipy.ndimage
import scipy.sparse

import localmd_amd
from localmd_amd import baseline as BL
from localmd_amd.pmdarray import PMDArray
from tests import baseline_ref as R

U24 = 2.0 ** -24


def test_sliding_emulations_equal_scipy_nearest():
    rng = np.random.default_rng(0)
    for n in (1, 2, 5, 16, 17, 50, 333):
        x = np.rint(20 * rng.standard_normal((n, 3))).astype(np.float32)       # ties
        x[:, 1] = rng.standard_normal(n).astype(np.float32)
        for h in (0, 1, 2, 7, 100):
            for is_max, filt in ((False, scipy.ndimage.minimum_filter1d), (True, scipy.ndimage.maximum_filter1d)):
                want = filt(x, 2 * h + 1, axis=0, mode="nearest")
                assert np.array_equal(R.sliding_view(x, h, is_max), want), (n, h, is_max)
                assert np.array_equal(R.sliding(x, h, is_max), want), (n, h, is_max)


def test_sliding_emulation_drops_nan_unless_the_window_is_all_nan():
    x = np.array([5, np.nan, np.nan, np.nan, 1, 7, np.nan, 3], np.float32)[:, None]
    lo = R.sliding(x, 1, False)[:, 0]
    assert np.array_equal(lo, np.array([5, 5, np.nan, 1, 1, 1, 3, 3], np.float32), equal_nan=True)
    hi = R.sliding(x, 1, True)[:, 0]
    assert np.array_equal(hi, np.array([5, 5, np.nan, 1, 7, 7, 7, 3], np.float32), equal_nan=True)
    assert np.all(np.isnan(R.sliding(np.full((4, 2), np.nan, np.float32), 100, False)))


def test_bin_chain_against_float64_means():
    """A chain of b - 1 additions and one division, each rounding relative to at most the bin's sum of magnitudes:
    within b 2^-24 mean |x| of the float64 mean."""
    rng = np.random.default_rng(1)
    y = (900 + 8 * rng.standard_normal((1000, 7))).astype(np.float32)
    for b in (1, 2, 32, 256):
        k = R.bin_chain(y, b)
        assert k.dtype == np.float32 and k.shape == (-(-1000 // b), 7)
        for i, s in enumerate(range(0, 1000, b)):
            blk = y[s:s + b].astype(np.float64)
            assert np.all(np.abs(k[i] - blk.mean(axis=0)) <= b * U24 * np.abs(blk).mean(axis=0)), (b, i)
    assert R.bin_chain(y, 1).tobytes() == y.tobytes()
    # the last bin is averaged over the frames it has
    assert np.array_equal(R.bin_chain(np.arange(10, dtype=np.float32)[:, None], 4)[:, 0], [1.5, 5.5, 8.5])
    assert np.array_equal(R.movie_knots(y, 32, block=256), R.bin_chain(y, 32))


def test_centres_and_interpolation():
    c = BL.bin_centres(1000, 32)
    assert len(c) == 32 and c[0] == 15.5 and c[1] == 47.5 and c[-1] == 995.5       # the last bin: 8 frames, 992 .. 999
    assert np.array_equal(c, R.centres(1000, 32))
    assert np.array_equal(BL.bin_centres(7, 1), np.arange(7.0))
    assert np.array_equal(BL.bin_centres(5, 256), [2.0])
    rng = np.random.default_rng(2)
    T, b = 1000, 32
    K = (100 + 30 * rng.standard_normal((32, 5))).astype(np.float32)
    t = np.arange(T)
    got = BL.interpolate(K, c, t)
    assert got.dtype == np.float32 and R.same_bits(got, R.baseline_frames(K, T, b, 0, T))
    assert np.all(got[:16] == K[0]) and np.all(got[996:] == K[-1])                 # before the first, after the last centre
    # one rounding in d (up to 2 max), one in w, one in the product, one in the sum: 2^-21 max(|K_j|, |K_j+1|)
    j = np.clip(np.searchsorted(c, t, side="right") - 1, 0, 30)
    w = np.clip((t - c[j]) / (c[j + 1] - c[j]), 0, 1)
    K64 = K.astype(np.float64)
    want = K64[j] + w[:, None] * (K64[j + 1] - K64[j])
    bound = 2.0 ** -21 * np.maximum(np.abs(K64[j]), np.abs(K64[j + 1]))
    assert np.all(np.abs(got - want) <= bound)
    # b = 1: every frame is a centre, the baseline at a frame is its knot, NaN and all
    K1 = rng.standard_normal((50, 3)).astype(np.float32)
    K1[7, 1] = np.nan
    assert BL.interpolate(K1, BL.bin_centres(50, 1), np.arange(50)).tobytes() == K1.tobytes()
    assert R.baseline_frames(K1, 50, 1, 0, 50).tobytes() == K1.tobytes()
    # a single bin: constant
    assert np.all(BL.interpolate(K[:1], BL.bin_centres(5, 256), np.arange(5)) == K[0])
    # a Baseline evaluates ranges of frames
    bl = BL.Baseline(K.reshape(32, 1, 5), b, 96, "maximin", "denoised", T)
    assert bl.frames(100, 230).tobytes() == got[100:230].reshape(130, 1, 5).tobytes()
    assert bl.frames().shape == (T, 1, 5) and np.array_equal(bl.centres, c)
    with pytest.raises(ValueError):
        bl.frames(10, 1001)


def test_window_to_half_rule():
    for b in (1, 2, 16, 256):
        for window in list(range(1, 70)) + [255, 256, 257, 3000, 3001]:
            h = BL.half_window(window, b)
            assert h == R.half_of(window, b), (window, b)
            assert (2 * h + 1) * b >= window and (h == 0 or (2 * h - 1) * b < window)
    assert BL.half_window(3000, 16) == 94 and (2 * 94 + 1) * 16 == 3024


def _pmd(T=40, d1=6, d2=5):
    rng = np.random.default_rng(3)
    u = scipy.sparse.random(d1 * d2, 4, density=0.5, random_state=1, format="coo", dtype=np.float32)
    return PMDArray(u, rng.standard_normal((4, 3)).astype(np.float32), np.ones(3, np.float32),
                    rng.standard_normal((3, T)).astype(np.float32), (T, d1, d2), "C", np.ones((d1, d2), np.float32),
                    np.ones((d1, d2), np.float32))


def test_argument_errors_come_before_any_device_work(tmp_path):
    """None of these reaches the device (this test runs without one) or creates a file."""
    pmd = _pmd()
    mov = np.zeros((40, 6, 5), np.float32)
    path = str(tmp_path / "out.npy")
    for kw in (dict(kind="residual"), dict(kind="nope"), dict(method="median"), dict(window=0), dict(window=-3),
               dict(window=2.5), dict(window=None), dict(temporal_bin=0), dict(temporal_bin=3), dict(temporal_bin=512),
               dict(temporal_bin=True), dict(kind="raw", movie=None)):
        args = dict(kind="denoised", window=10, temporal_bin=4, method="maximin", movie=mov)
        args.update(kw)
        movie = args.pop("movie")
        with pytest.raises(ValueError):
            localmd_amd.rolling_baseline(pmd, movie, **args)
        with pytest.raises(ValueError):
            localmd_amd.dff_movie(pmd, path, movie, **args)
    with pytest.raises(ValueError, match="output"):
        localmd_amd.dff_movie(pmd, path, window=10, output="ratio")
    with pytest.raises(ValueError, match="window"):
        localmd_amd.dff_movie(pmd, path)
    with pytest.raises(ValueError, match="suffix"):
        localmd_amd.dff_movie(pmd, str(tmp_path / "out.bin"), window=10)
    with pytest.raises(ValueError, match="shape"):
        localmd_amd.rolling_baseline(pmd, np.zeros((41, 6, 5), np.float32), kind="raw", window=10)
    with pytest.raises(TypeError):
        localmd_amd.rolling_baseline(object(), window=10)
    with pytest.raises(ValueError, match="no frames"):
        localmd_amd.rolling_baseline(_pmd(T=0), window=10)
    with pytest.raises(ValueError, match="no frames"):
        localmd_amd.dff_movie(_pmd(T=0), path, window=10)
    for kw in (dict(window=0), dict(temporal_bin=6), dict(method="x"), dict(output="x")):
        args = dict(window=5)
        args.update(kw)
        with pytest.raises(ValueError):
            localmd_amd.trace_baseline(np.zeros((2, 30)), **args)
    with pytest.raises(ValueError):
        localmd_amd.trace_baseline(np.zeros(30), window=5)
    with pytest.raises(ValueError, match="no frames"):
        localmd_amd.trace_baseline(np.zeros((2, 0)), window=5)
    assert not list(tmp_path.iterdir())
    assert callable(PMDArray.baseline) and callable(PMDArray.dff)


def test_too_many_frames_are_refused():
    with pytest.raises(ValueError, match="2\\^23"):
        BL._check_frames(2 ** 23, "the decomposition")
    BL._check_frames(2 ** 23 - 1, "the decomposition")


def test_baseline_checks(tmp_path):
    pmd = _pmd()
    path = str(tmp_path / "out.npy")
    good = BL.Baseline(np.ones((10, 6, 5), np.float32), 4, 12, "maximin", "denoised", 40)
    assert "10 knots of 4 frames" in repr(good) and good.window_frames == 12
    BL._check_baseline(good, (40, 6, 5), "denoised")
    bad = [BL.Baseline(np.ones((10, 6, 5), np.float32), 4, 12, "maximin", "raw", 40),          # another kind
           BL.Baseline(np.ones((10, 6, 5), np.float32), 4, 12, "maximin", "denoised", 39),     # another movie length
           BL.Baseline(np.ones((5, 6, 5), np.float32), 4, 12, "maximin", "denoised", 40),      # knots of another bin
           BL.Baseline(np.ones((10, 5, 6), np.float32), 4, 12, "maximin", "denoised", 40),     # another field of view
           BL.Baseline(np.ones((10, 6, 5), np.float64), 4, 12, "maximin", "denoised", 40),     # not float32
           BL.Baseline(np.ones((14, 6, 5), np.float32), 3, 12, "maximin", "denoised", 40)]     # not a power of two
    for b in bad:
        with pytest.raises(ValueError):
            localmd_amd.dff_movie(pmd, path, baseline=b)
    with pytest.raises(TypeError):
        localmd_amd.dff_movie(pmd, path, baseline=np.ones((10, 6, 5), np.float32))
    with pytest.raises(ValueError, match="not both"):
        localmd_amd.dff_movie(pmd, path, baseline=good, window=12)
    assert not list(tmp_path.iterdir())


def test_memory_plan():
    D = 512 * 512
    n_bins = 625                                    # 10000 frames in bins of 16
    ranges, work = BL.filter_plan(n_bins, D)
    assert ranges[0][0] == 0 and ranges[-1][1] == D and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    cols = ranges[0][1]
    assert cols % 256 == 0 and work == n_bins * cols and 4 * work <= BL.WORK_BYTES < 4 * n_bins * (cols + 256)
    assert len(ranges) == 3
    # a small problem takes one call with a workspace of its own size (columns rounded up to 4)
    assert BL.filter_plan(141, 1921) == ([(0, 1921)], 141 * 1924)
    # the longest series there can be still fits: ranges of a multiple of 4 columns
    ranges, work = BL.filter_plan(2 ** 23 - 1, 10)
    assert 4 * work <= BL.WORK_BYTES and ranges == [(0, 8), (8, 10)]
    # the terms that grow with the movie's length: knots, filter output, workspace
    assert BL.knot_bytes(10000, D, 16) == 2 * 4 * n_bins * D + 4 * n_bins * cols
    kw = dict(D=D, nb=10000, esize=2, n_cols=3000, rank=200, n_entries=9000, n_a=10 ** 6, n_patches=D // 64,
              host_source=True, n_batches=2, factors_on_device=False)
    for kind in ("raw", "denoised"):
        a = BL.baseline_device_bytes(T=10000, temporal_bin=16, kind=kind, **kw)
        b = BL.baseline_device_bytes(T=20000, temporal_bin=16, kind=kind, **kw)
        c = BL.baseline_device_bytes(T=20000, temporal_bin=32, kind=kind, **kw)
        assert b - a == BL.knot_bytes(20000, D, 16) - BL.knot_bytes(10000, D, 16) > 0 and c == a
        assert BL.baseline_device_bytes(T=10000, temporal_bin=16, kind=kind, host_dest=True, **kw) - a == 2 * 1024 * D * 4
    with pytest.raises(ValueError, match="raise temporal_bin"):
        BL.check_fit("rolling_baseline", 10 ** 12, 10 ** 11)
    BL.check_fit("rolling_baseline", 10, 10)


def test_opening_follows_a_decaying_baseline_under_short_transients():
    """Noise-free, b = 1: a decreasing baseline B with positive bumps of L < 2 h + 1 frames.  The minimum filter removes
    the bumps and runs ahead of B by up to h frames, the maximum filter brings it back: away from the ends
    B[t] <= out[t] <= B[t - L]."""
    n, L, h = 4000, 20, 30
    t = np.arange(n)
    B = (100 * np.exp(-t / 800.0) + 50).astype(np.float32)
    x = B.copy()
    for s in range(100, n - 100, 150):
        x[s:s + L] += 40
    out = R.filtered(x[:, None], h, "maximin")[:, 0]
    inner = np.arange(2 * h, n - 2 * h)
    assert np.all(B[inner] <= out[inner]) and np.all(out[inner] <= B[inner - L])
    assert not np.all(R.filtered(x[:, None], h, "minimum")[inner, 0] >= B[inner])      # the minimum alone undershoots
