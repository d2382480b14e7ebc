"""Host-side tests of the percentile baseline (no GPU): the window-sort reference of tests/baseline_quantile_ref.py
against scipy.ndimage, the rank rule against percentile_filter, the emulation of the kernel's incremental rule against
the window sort, the argument checks of method="percentile" and q, the Baseline object, the memory plan, and what the
method is for: a percentile is not biased by the knots' noise as an extremum is."""
import os
import re

import numpy as np
import pytest
import scipy.ndimage

import localmd_amd
from localmd_amd import baseline as BL
from localmd_amd.quantiles import float_keys
from tests import baseline_quantile_ref as Q
from tests import baseline_ref as R
from tests.test_baseline_host import _pmd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sliding_rank_equals_scipy_rank_filter():
    """The (W, 1) footprint on the (n, N) matrix, mode "nearest"; h below, equal to and far above n."""
    rng = np.random.default_rng(0)
    for n in (1, 2, 7, 40):
        for h in sorted({0, 1, 3, n - 1, n, n + 1, 3 * n, 10 * n + 3} - {-1}):
            W = 2 * h + 1
            x = np.stack([rng.standard_normal(n), rng.integers(-3, 4, n), np.arange(n), -np.arange(n)], axis=1).astype(np.float32)
            ranks = sorted({0, 1 % W, h, W - 1, Q.rank_of(h, 0.08)})
            got = Q.sliding_ranks(x, h, ranks)
            for k in ranks:
                want = scipy.ndimage.rank_filter(x, rank=k, size=(W, 1), mode="nearest")
                assert got[k].tobytes() == want.tobytes(), (n, h, k)


def test_sliding_rank_orders_zeros_nan_and_inf_by_key():
    x = np.array([[0.0], [np.nan], [-0.0], [np.inf], [-np.inf], [-1.0], [np.nan]], np.float32)
    s = [Q.sliding_rank(x, 10, k)[0, 0] for k in range(21)]
    # the window of output 0 is the whole series with the first row 11 times and the last (a NaN) 5 times: 6 NaNs in all
    want = [-np.inf, -1.0, -0.0] + [0.0] * 11 + [np.inf] + [np.nan] * 6
    assert np.array_equal(np.array(s, np.float32).view(np.uint32)[:15], np.array(want, np.float32).view(np.uint32)[:15])
    assert np.all(np.isnan(s[15:])) and np.signbit(s[2]) and not np.signbit(s[3])
    # rank 0 drops NaN unless the whole window is NaN; the top rank lets it win
    y = np.array([[1.0, np.nan], [np.nan, np.nan], [3.0, np.nan]], np.float32)
    lo, hi = Q.sliding_rank(y, 1, 0), Q.sliding_rank(y, 1, 2)
    assert np.array_equal(lo[:, 0], [1, 1, 3]) and np.all(np.isnan(lo[:, 1])) and np.all(np.isnan(hi))


def test_weighted_rank_equals_sliding_rank():
    """The reference for windows too long to build (the GPU tests use it at half = 2^30 - 1) against the window sort."""
    rng = np.random.default_rng(3)
    for n in (1, 2, 5):
        for h in (0, 1, n, 4 * n + 1):
            x = Q.series(rng, n, len(Q.SERIES_KINDS), h)
            for k in sorted({0, h, 2 * h}):
                assert R.same_bits(Q.weighted_rank(x, h, k), Q.sliding_rank(x, h, k)), (n, h, k)


def test_rank_rule_is_that_of_percentile_filter():
    rng = np.random.default_rng(1)
    x = rng.permutation(200).reshape(40, 5).astype(np.float32)            # distinct values: the rank shows
    for h in (0, 1, 3, 25):
        W = 2 * h + 1
        for q in (0.0, 0.08, 0.5, 0.92, 1.0):
            k = BL.percentile_rank(h, q)
            assert k == Q.rank_of(h, q) and 0 <= k <= W - 1
            want = scipy.ndimage.percentile_filter(x, 100 * q, size=(W, 1), mode="nearest")
            assert Q.sliding_rank(x, h, k).tobytes() == want.tobytes(), (h, q)
            assert Q.filtered_percentile(x, h, q).tobytes() == want.tobytes()
    assert BL.percentile_rank(94, 0.08) == 15 and BL.percentile_rank(1500, 0.08) == 240
    assert BL.percentile_rank(3, 1.0) == 6 and BL.percentile_rank(0, 0.5) == 0


def test_slice_constant_matches_the_header():
    header = open(os.path.join(ROOT, "include", "pmd_hip.h")).read()
    assert int(re.search(r"#define PMD_SLIDING_QUANTILE_SLICE (\d+)", header).group(1)) == BL.QUANTILE_SLICE >= 64


@pytest.mark.parametrize("S", [4, 7])
def test_incremental_rule_equals_the_window_sort(S):
    """The kernel's rule (emulate: its own assertions check that the answer moves by one distinct value, down with
    cl == rank + 1 or up with cl + ce == rank) with every output in turn the first of a slice."""
    rng = np.random.default_rng(2 + S)
    cases = 0
    for n in (1, 2, 5, 13):
        for h in sorted({0, 1, 2, n - 1, n, 3 * n} - {-1}):
            W = 2 * h + 1
            x = Q.series(rng, n, len(Q.SERIES_KINDS), h)
            ranks = sorted({0, 1 % W, h, max(0, W - 2), W - 1, Q.rank_of(h, 0.08)})
            want = Q.sliding_ranks(x, h, ranks)
            for k in ranks:
                for offset in range(min(S, n)):
                    for c in range(x.shape[1]):
                        got = Q.emulate(x[:, c], h, k, S, offset)
                        assert R.same_bits(got, want[k][:, c]), (n, h, k, offset, Q.SERIES_KINDS[c])
                        cases += 1
    assert cases > 2000


def test_incremental_rule_work_is_bounded_by_the_rows_the_window_holds():
    """Element visits per output: at most one scan of min(W, n) + 2 rows, plus 33 per slice; whatever half is."""
    rng = np.random.default_rng(5)
    n, S = 300, BL.QUANTILE_SLICE
    x = rng.standard_normal(n).astype(np.float32)
    want = {}
    for h in (10, 94, 400, 10 ** 6):
        W = 2 * h + 1
        stats = {}
        got = Q.emulate(x, h, Q.rank_of(h, 0.08), S, 0, stats)
        slices = -(-n // S)
        assert stats["scans"] <= n + 32 * slices
        assert stats["visits"] <= stats["scans"] * (min(W, n) + 2)
        want[h] = got
    # with half >= n every window holds the whole series: replicated edges decide the rest
    assert np.array_equal(want[400], Q.sliding_rank(x[:, None], 400, Q.rank_of(400, 0.08))[:, 0])
    keys = np.sort(float_keys(x))
    assert set(float_keys(want[10 ** 6]).tolist()) <= set(keys.tolist())


def test_argument_errors_come_before_any_device_work(tmp_path):
    pmd = _pmd()
    path = str(tmp_path / "out.npy")
    for kw in (dict(method="maximin", q=0.1), dict(method="minimum", q=0.5), dict(q=-0.01), dict(q=1.01), dict(q=float("nan")),
               dict(q=True), dict(q=np.bool_(False)), dict(q="0.1"), dict(q=[0.1]), dict(method="median"),
               dict(method="median", q=0.5), dict(method="Percentile")):
        args = dict(window=10, temporal_bin=4, method="percentile")
        args.update(kw)
        with pytest.raises(ValueError):
            localmd_amd.rolling_baseline(pmd, **args)
        with pytest.raises(ValueError):
            localmd_amd.dff_movie(pmd, path, **args)
        with pytest.raises(ValueError):
            localmd_amd.trace_baseline(np.zeros((2, 30)), **args)
    with pytest.raises(ValueError, match="maximin.*minimum.*percentile"):
        localmd_amd.rolling_baseline(pmd, window=10, method="median")
    good = BL.Baseline(np.ones((10, 6, 5), np.float32), 4, 12, "percentile", "denoised", 40, q=0.08)
    with pytest.raises(ValueError, match="q="):
        localmd_amd.dff_movie(pmd, path, baseline=good, q=0.08)
    with pytest.raises(ValueError, match="not both"):
        localmd_amd.dff_movie(pmd, path, baseline=good, window=12)
    assert not list(tmp_path.iterdir())
    assert BL.METHODS == ("maximin", "minimum") and BL.ALL_METHODS == ("maximin", "minimum", "percentile")
    assert BL._check_method("percentile", None) == ("percentile", 0.08)
    assert BL._check_method("percentile", 1) == ("percentile", 1.0) and BL._check_method("minimum", None) == ("minimum", None)
    assert BL._check_method("percentile", np.float32(0.5)) == ("percentile", 0.5)
    with pytest.raises(ValueError, match="too long"):
        BL._check_half(2 ** 30, "percentile")
    assert BL._check_half(2 ** 30 - 1, "percentile") == 2 ** 30 - 1 and BL._check_half(2 ** 40, "minimum") == 2 ** 40


def test_percentile_baseline_object():
    knots = np.ones((10, 6, 5), np.float32)
    bl = BL.Baseline(knots, 4, 12, "percentile", "denoised", 40, q=0.08)
    assert bl.q == 0.08 and "percentile q=0.08 over 12 frames" in repr(bl)
    BL._check_baseline(bl, (40, 6, 5), "denoised")
    old = BL.Baseline(knots, 4, 12, "maximin", "denoised", 40)          # positional construction as before
    assert old.q is None and "maximin over 12 frames" in repr(old)
    BL._check_baseline(old, (40, 6, 5), "denoised")
    for bad in (BL.Baseline(knots, 4, 12, "percentile", "denoised", 40),               # no q
                BL.Baseline(knots, 4, 12, "percentile", "denoised", 40, q=1.5),
                BL.Baseline(knots, 4, 12, "maximin", "denoised", 40, q=0.5),
                BL.Baseline(knots, 4, 12, "median", "denoised", 40, q=0.5)):
        with pytest.raises(ValueError):
            BL._check_baseline(bad, (40, 6, 5), "denoised")


def test_memory_plan():
    D = 512 * 512
    n_bins = 625
    ranges, work = BL.filter_plan(n_bins, D)
    old = 2 * 4 * n_bins * D + 4 * work
    assert BL.knot_bytes(10000, D, 16) == BL.knot_bytes(10000, D, 16, "maximin", 94) == BL.knot_bytes(10000, D, 16, "minimum") == old
    # the percentile filter: the two matrices and its own workspace over the same column ranges, which is none
    assert BL.quantile_work_floats(n_bins, ranges[0][1], 94) == 0
    assert BL.knot_bytes(10000, D, 16, "percentile", 94) == 2 * 4 * n_bins * D
    kw = dict(T=10000, D=D, temporal_bin=16, nb=10000, esize=2, n_cols=3000, rank=200, n_entries=9000, n_a=10 ** 6,
              n_patches=D // 64, host_source=True, n_batches=2, factors_on_device=False)
    for kind in ("raw", "denoised"):
        a = BL.baseline_device_bytes(kind=kind, **kw)
        assert a == BL.baseline_device_bytes(kind=kind, method="minimum", half=94, **kw)
        assert a - BL.baseline_device_bytes(kind=kind, method="percentile", half=94, **kw) == 4 * work


def test_a_percentile_is_closer_to_the_floor_than_the_minimum():
    """A constant floor plus Gaussian noise: the running median sits at the floor up to the noise of a median of W
    knots, the running minimum several noise standard deviations below; at every knot."""
    rng = np.random.default_rng(7)
    floor, h = np.float32(100.0), 94
    knots = (floor + rng.standard_normal((625, 4))).astype(np.float32)
    med = Q.filtered_percentile(knots, h, 0.5)
    low = R.filtered(knots, h, "minimum")
    assert np.all(np.abs(med - floor) < np.abs(low - floor))
    # away from the ends, where no window holds replicated copies of an end knot: a median of 189 draws has a standard
    # deviation of 1.25 / sqrt(189) = 0.09, and the least of 189 draws lies 2.7 below on average
    inner = slice(h, 625 - h)
    assert np.abs(med[inner] - floor).max() < 0.5 and (floor - low[inner]).min() > 1.5
