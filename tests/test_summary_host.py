"""Host side of localmd_amd.summary_images (no GPU): argument errors before any device work and before the movie is read,
the float64 finish of the moments and of the peak-to-noise ratio against NumPy, a NumPy emulation of the kernel's temporal
binning (the documented order of its fp32 sums) against float64 bin means, and a device-memory plan that does not depend
on the movie's length."""
import numpy as np
import pytest

import localmd_amd
from localmd_amd import summary as SM
from localmd_amd._stream import block_plan
from localmd_amd.maps import GAMMA
from localmd_amd.pmdarray import PMDArray
from tests.test_traces_host import _Untouchable, _pmd, no_device  # noqa: F401 - no_device is a fixture

T, D1, D2 = 300, 6, 7
SLICE = 256          # frames per slice of pmd_pixel_stats_accumulate (include/pmd_hip.h)


def test_reexported():
    assert localmd_amd.summary_images is SM.summary_images
    assert "summary_images" in localmd_amd.__all__
    assert callable(PMDArray.summary)
    assert SM.STATS == ("mean", "std", "min", "max", "argmin", "argmax", "skewness", "kurtosis", "pnr")


def test_summary_object():
    img = np.zeros((D1, D2), np.float32)
    s = SM.Summary(raw={"max": img}, stats=("max",), temporal_bin=4)
    assert s.denoised is None and s.residual is None and s.raw["max"] is img
    assert s.stats == ("max",) and s.temporal_bin == 4
    assert repr(s) == "Summary(raw; max; temporal_bin=4)"


def _bad_calls():
    mov = _Untouchable((T, D1, D2))
    return [
        dict(kinds="noise"),
        dict(kinds=()),
        dict(kinds=("raw", "raw"), movie=mov),
        dict(kinds=3),
        dict(stats="median"),
        dict(stats=()),
        dict(stats=("max", "max")),
        dict(stats=5),
        dict(temporal_bin=0),
        dict(temporal_bin=3),
        dict(temporal_bin=2048),
        dict(temporal_bin=-2),
        dict(temporal_bin=2.0),
        dict(temporal_bin=True),
        dict(temporal_bin="2"),
        dict(kinds=("raw",)),                                               # raw without a movie
        dict(kinds=("denoised", "residual")),                               # residual without a movie
        dict(kinds="raw", movie=_Untouchable((T, D1, D2 + 1))),
        dict(kinds="raw", movie=np.zeros((T - 1, D1, D2), np.float32)),
        dict(kinds="denoised", movie=np.zeros((T - 1, D1, D2), np.float32)),
    ]


def test_argument_errors_before_any_device_work(no_device):  # noqa: F811
    pmd = _pmd(T, D1, D2)
    for kw in _bad_calls():
        with pytest.raises(ValueError):
            localmd_amd.summary_images(pmd, **kw)
        with pytest.raises(ValueError):
            pmd.summary(**kw)
    with pytest.raises(TypeError):
        localmd_amd.summary_images(np.zeros((T, D1, D2)))
    # no frames: extrema of nothing do not exist
    empty = _pmd(0, D1, D2)
    with pytest.raises(ValueError, match="no frames"):
        localmd_amd.summary_images(empty)
    with pytest.raises(ValueError, match="no frames"):
        empty.summary(_Untouchable((0, D1, D2)), kinds="raw", stats="max")


# ---- the float64 finish --------------------------------------------------------------------------------------------
def _power_sums(y, centre):
    z = y - centre[None, :]
    return np.stack([(z ** p).sum(axis=0) for p in (1, 2, 3, 4)])


def test_finish_moments_against_numpy():
    rng = np.random.default_rng(0)
    n, N = 2000, 40
    y = 900.0 + 8.0 * rng.gamma(2.0, 1.0, (n, N))                      # skewness about 1.4, excess kurtosis about 3
    sd = y.std(axis=0)
    centre = y.mean(axis=0) + np.linspace(-10.0, 10.0, N) * sd         # the centre up to 10 std away from the mean
    got = SM.finish_moments(_power_sums(y, centre), n, centre)
    d = y - y.mean(axis=0)
    m2, m3, m4 = ((d ** p).mean(axis=0) for p in (2, 3, 4))
    want = {"mean": np.mean(y, axis=0), "std": np.std(y, axis=0), "skewness": m3 / m2 ** 1.5,
            "kurtosis": m4 / m2 ** 2 - 3.0}
    assert sorted(got) == sorted(want)
    assert np.abs(want["skewness"]).min() > 0.5 and np.abs(want["kurtosis"]).min() > 0.5
    for k in want:
        assert got[k].dtype == np.float64 and got[k].shape == (N,)
        np.testing.assert_allclose(got[k], want[k], rtol=1e-10, atol=0, err_msg=k)


def test_finish_moments_zeroes_constant_pixels_and_the_variance_floor():
    n = 1000
    rng = np.random.default_rng(1)
    y = np.empty((n, 4))
    y[:, 0] = 900.0                                                    # constant, at the centre
    y[:, 1] = 907.0                                                    # constant, away from it
    y[:, 2] = 907.0 + 1e-3 * rng.standard_normal(n)                    # variance 1e-6 under z^2 = 49: below the floor
    y[:, 3] = 907.0 + 1.0 * rng.standard_normal(n)                     # a pixel with variance, for contrast
    centre = np.full(4, 900.0)
    S = _power_sums(y, centre)
    var = S[1] - S[0] ** 2 / n
    assert var[2] > 0 and var[2] <= 3 * GAMMA * S[1][2] and var[3] > 3 * GAMMA * S[1][3]
    got = SM.finish_moments(S, n, centre)
    for k in ("std", "skewness", "kurtosis"):
        assert np.array_equal(got[k][:3], np.zeros(3)), k
    np.testing.assert_allclose(got["mean"], y.mean(axis=0), rtol=1e-14)
    assert abs(got["std"][3] - y[:, 3].std()) < 1e-9 and got["skewness"][3] != 0 and got["kurtosis"][3] != 0
    # the perturbed sums of a constant pixel (what fp32 block sums leave behind) still give zeros, not noise
    S1 = S[:, 1:2] * (1.0 + GAMMA * np.array([[0.5], [-0.5], [0.3], [-0.2]]))
    noisy = SM.finish_moments(S1, n, centre[1:2])
    assert noisy["std"][0] == 0 and noisy["skewness"][0] == 0 and noisy["kurtosis"][0] == 0


def test_finish_pnr_is_zero_without_a_usable_noise():
    peak = np.array([950, 950, 950, 950, 950, 900], np.float32)
    mean = np.array([900.25, 900, 900, 900, 900, 950], np.float64)
    noise = np.array([8.0, 0.0, np.nan, np.inf, -1.0, 4.0])
    got = SM.finish_pnr(peak, mean, noise)
    assert got.dtype == np.float32
    assert np.array_equal(got, np.array([(950 - 900.25) / 8.0, 0, 0, 0, 0, -12.5], np.float32))
    assert np.array_equal(SM.finish_pnr(peak, mean, noise.astype(np.float32)), got)


# ---- the kernel's binning, emulated ----------------------------------------------------------------------------------
def emulate_bins(y, bin):
    """The fp32 values pmd_pixel_stats_accumulate takes the extrema of, for one call on the (n, N) float32 block ``y``
    (include/pmd_hip.h): (first frame of every bin, (bins, N) float32).  bin == 1: the frames themselves.  A bin of at
    most 256 frames: one fp32 chain over its frames in ascending order starting from the first frame's value, divided in
    fp32 by the number of frames.  A bin of 512 or 1024 frames: the 256-frame slices of the bin are summed so, the slice
    sums are added in ascending order starting from the first, then divided."""
    y = np.asarray(y, np.float32)
    n = y.shape[0]
    starts = np.arange(0, n, bin)
    if bin == 1:
        return starts, y.copy()

    def chain(a):
        s = a[0].copy()
        for r in a[1:]:
            s = (s + r).astype(np.float32)
        return s

    out = np.empty((len(starts), y.shape[1]), np.float32)
    for i, b in enumerate(starts):
        e = min(n, b + bin)
        s = chain(y[b:min(e, b + SLICE)])
        for a in range(b + SLICE, e, SLICE):
            s = (s + chain(y[a:min(e, a + SLICE)])).astype(np.float32)
        out[i] = s / np.float32(e - b)
    return starts, out


@pytest.mark.parametrize("bin", [1, 2, 8, 256, 512, 1024])
def test_emulated_binning_is_exact_on_integer_data(bin):
    """Integer frames below 2^12 sum to integers below 2^22 over 1024 frames: every fp32 sum is exact whatever its
    order, so the emulated bin value is the float64 bin mean rounded once."""
    rng = np.random.default_rng(bin)
    for n in (1, 7, 300, 1000, 1024):
        y = rng.integers(0, 4096, (n, 5)).astype(np.float32)
        starts, got = emulate_bins(y, bin)
        assert np.array_equal(starts, np.arange(0, n, bin)) and got.dtype == np.float32
        want = np.stack([y[b:b + bin].astype(np.float64).mean(axis=0) for b in starts]).astype(np.float32)
        assert np.array_equal(got, want), n


# ---- the memory plan -------------------------------------------------------------------------------------------------
def _plan_bytes(T, fbs, **kw):
    plan = block_plan(T, fbs)
    args = dict(D=4096, nb=plan[0][1] - plan[0][0], esize=2, n_raw=1, n_expand=2, need_ext=True, need_arg=True,
                need_mom=True, n_cols=300, rank=12, n_entries=900, n_a=50000, n_patches=64, needs_movie=True,
                host_source=True, n_batches=len(plan), factors_on_device=False)
    args.update(kw)
    return SM.summary_device_bytes(**args)


def test_device_bytes_do_not_grow_with_the_movie():
    from localmd_amd._stream import BLOCK, batch_buffer_bytes

    a = _plan_bytes(10 ** 4, 4096)
    assert a == _plan_bytes(10 ** 6, 4096)
    D = 4096
    # the state: 8 bytes of extrema, 8 of frame numbers, 32 of power sums per pixel and kind, only when needed
    assert a - _plan_bytes(10 ** 4, 4096, need_arg=False) == 8 * 3 * D
    assert a - _plan_bytes(10 ** 4, 4096, need_ext=False, need_arg=False) == 16 * 3 * D
    assert a - _plan_bytes(10 ** 4, 4096, need_mom=False) == 32 * 3 * D
    assert a - _plan_bytes(10 ** 4, 4096, n_expand=1) == (48 + 4) * D + 4 * BLOCK * D
    assert a - _plan_bytes(10 ** 4, 4096, needs_movie=False) == batch_buffer_bytes(4096, D, 2, True, 3)
    assert _plan_bytes(10 ** 4, 4096, factors_on_device=True) == a - 4 * 300 * 12
    with pytest.raises(TypeError):
        SM.summary_device_bytes(4096, 4096, 2)                     # keyword-only: no silent mis-ordering
    with pytest.raises(ValueError):
        SM.check_fit("summary_images", a, a - 1)
