"""Host side of localmd_amd.regressor_maps (no GPU): argument errors before any device work and before the movie is read,
event_regressors against hand-written arrays, the centred and normalised regressors of the correlation, the Pearson
finish against NumPy, and a device-memory plan that does not depend on the movie's length."""
import numpy as np
import pytest

import localmd_amd
from localmd_amd import maps as MP
from localmd_amd.pmdarray import PMDArray
from tests.test_traces_host import _Untouchable, _pmd, no_device  # noqa: F401 - no_device is a fixture

T, D1, D2 = 300, 6, 7


def test_reexported():
    assert localmd_amd.regressor_maps is MP.regressor_maps and localmd_amd.event_regressors is MP.event_regressors
    assert "regressor_maps" in localmd_amd.__all__ and "event_regressors" in localmd_amd.__all__
    assert callable(PMDArray.maps)


def _bad_calls():
    mov = _Untouchable((T, D1, D2))
    ok = np.random.default_rng(0).standard_normal((2, T))
    nan_x, inf_x, zero_sum, huge = ok.copy(), ok.copy(), ok.copy(), ok.copy()
    nan_x[1, 7] = np.nan
    inf_x[0, 0] = -np.inf
    zero_sum[1] = 0.0
    zero_sum[1, :2] = (1.0, -1.0)
    huge[0, 3] = 1e60                                                             # finite, but not in float32
    return [
        dict(x=ok, kinds="noise"),
        dict(x=ok, kinds=()),
        dict(x=ok, kinds=("raw", "raw"), movie=mov),
        dict(x=ok, kinds=3),
        dict(x=ok, stat="median"),
        dict(x=ok, stat=("sum",)),
        dict(x=ok[:, :T - 1]),                                                    # wrong T
        dict(x=ok[0, :T - 1]),
        dict(x=np.zeros((0, T))),                                                 # K = 0
        dict(x=np.zeros((2, 3, T))),
        dict(x=ok.astype(np.complex64)),
        dict(x=nan_x),
        dict(x=inf_x),
        dict(x=huge),
        dict(x=zero_sum, stat="mean"),
        dict(x=ok, kinds=("raw",)),                                               # raw without a movie
        dict(x=ok, kinds=("denoised", "residual")),                               # residual without a movie
        dict(x=ok, kinds="denoised", stat="correlation"),                         # correlation without a movie
        dict(x=ok, kinds="raw", movie=_Untouchable((T, D1, D2 + 1))),
        dict(x=ok, kinds="raw", movie=np.zeros((T - 1, D1, D2), np.float32)),
        dict(x=ok, kinds="denoised", movie=np.zeros((T - 1, D1, D2), np.float32)),
    ]


def test_argument_errors_before_any_device_work(no_device):  # noqa: F811
    pmd = _pmd(T, D1, D2)
    for kw in _bad_calls():
        kw = dict(kw)
        x = kw.pop("x")
        with pytest.raises(ValueError):
            localmd_amd.regressor_maps(pmd, x, **kw)
        with pytest.raises(ValueError):
            pmd.maps(x, **kw)
    with pytest.raises(TypeError):
        localmd_amd.regressor_maps(np.zeros((T, D1, D2)), np.ones((1, T)))


def test_sum_accepts_the_row_that_mean_refuses():
    x = np.zeros((1, T))
    x[0, :2] = (1.0, -1.0)
    assert np.array_equal(MP.prepare_regressors(x, T), x)
    assert MP.prepare_regressors(x[0], T).shape == (1, T)                          # (T,) is K = 1
    assert MP.prepare_regressors(np.ones((2, T), bool), T).dtype == np.float64


def test_event_regressors_against_hand_written_rows():
    got = MP.event_regressors(8, [0, 3, 7], [-1, 0, 2])
    want = np.array([[0, 0, 0.5, 0, 0, 0, 0.5, 0],                # lag -1: the event at 0 falls off the front
                     [1 / 3, 0, 0, 1 / 3, 0, 0, 0, 1 / 3],
                     [0, 0, 0.5, 0, 0, 0.5, 0, 0]])               # lag 2: the event at 7 falls off the end
    assert got.dtype == np.float64 and got.shape == (3, 8)
    assert np.array_equal(got, want)
    assert np.array_equal(MP.event_regressors(5, np.array([4]), np.array([0])), [[0, 0, 0, 0, 1.0]])
    for events, lags in (([0, 1], [-2]), ([6], [2, 0]), ([], [0]), ([1], [])):
        with pytest.raises(ValueError):
            MP.event_regressors(8, events, lags)
    with pytest.raises(ValueError):
        MP.event_regressors(8, [0.5], [0])


def test_normalized_regressors_have_mean_zero_and_norm_one():
    rng = np.random.default_rng(1)
    x = np.stack([rng.standard_normal(2500), 900.0 + 8.0 * rng.standard_normal(2500), 1e6 + rng.standard_normal(2500),
                  np.full(2500, 7.25), np.zeros(2500)])
    n = MP.normalized_regressors(x)
    assert n.dtype == np.float64
    assert np.all(np.abs(n.mean(axis=1)) < 1e-17)
    assert np.all(np.abs((n[:3] * n[:3]).sum(axis=1) - 1.0) < 1e-13)
    assert np.array_equal(n[3:], np.zeros((2, 2500)))                              # rows without variance
    for k in range(3):
        assert abs(np.corrcoef(n[k], x[k])[0, 1] - 1.0) < 1e-9


def test_centring_vector_is_dyadic_and_close_to_the_mean():
    rng = np.random.default_rng(3)
    mean = np.concatenate([rng.uniform(500, 1500, 20), rng.uniform(0.2, 0.8, 20), [40000.25, 3.0, 7.5, 1e9]])
    std = np.concatenate([rng.uniform(2, 20, 20), rng.uniform(0.005, 0.02, 20), [8.0, 0.0, np.nan, 1.0]])
    pmd = _pmd(T, 4, 11)
    pmd.mean_img, pmd.var_img = mean.reshape(4, 11), std.reshape(4, 11)
    c = MP.centring_vector(pmd)
    assert c.dtype == np.float32 and c.shape == (44,)
    m32, s32 = mean.astype(np.float32), std.astype(np.float32)
    assert np.all(np.abs(c[:41].astype(np.float64) - m32[:41]) <= s32[:41].astype(np.float64) / 16)
    q = np.exp2(np.floor(np.log2(s32[:41].astype(np.float64) / 8)))
    assert np.array_equal(np.rint(c[:41] / q), c[:41] / q) and np.all(q <= s32[:41] / 8) and np.all(q > s32[:41] / 16)
    assert np.array_equal(c[:20], np.rint(c[:20] * 4) / 4)                  # std >= 2: multiples of 1/4 at the finest
    assert c[40] == 40000.0 and np.array_equal(c[41:], m32[41:])           # no usable std: the mean itself


def test_pearson_finish_matches_numpy_and_zeroes_constants():
    rng = np.random.default_rng(2)
    n = 500
    x = MP.normalized_regressors(rng.standard_normal((3, n))).astype(np.float32).astype(np.float64)
    z = rng.standard_normal((n, 6)) + np.arange(6)[None, :]
    z[:, 4] = 3.0                                                                  # a constant pixel
    r = MP._pearson(x @ z, z.sum(axis=0), (z * z).sum(axis=0), x.sum(axis=1), (x * x).sum(axis=1), n)
    assert r.dtype == np.float32 and r.shape == (3, 6)
    assert np.array_equal(r[:, 4], np.zeros(3, np.float32))
    for k in range(3):
        for p in (0, 1, 2, 3, 5):
            assert abs(r[k, p] - np.corrcoef(x[k], z[:, p])[0, 1]) < 2e-7
    zero_x = MP._pearson(np.zeros((1, 6)), z.sum(axis=0), (z * z).sum(axis=0), np.zeros(1), np.zeros(1), n)
    assert np.array_equal(zero_x, np.zeros((1, 6), np.float32))


def test_device_bytes_count_the_plan():
    """The terms of the memory plan: the fp64 accumulators and moments of each kernel-accumulated kind, the batch
    buffers, one expanded block per expanded panel; the length of the movie is not an argument."""
    from localmd_amd._stream import BLOCK, batch_buffer_bytes

    D, K = 4096, 70
    args = dict(D=D, nb=4096, esize=2, K=K, n_acc=2, n_expand=1, n_cols=300, rank=12, n_entries=900, n_a=50000,
                n_patches=64, needs_movie=True, host_source=True, n_batches=10, factors_on_device=False,
                factor_sums=False)
    a = MP.maps_device_bytes(**args)
    assert a - MP.maps_device_bytes(**dict(args, n_acc=1)) == 8 * (K + 2) * D
    assert MP.maps_device_bytes(**dict(args, n_expand=2)) - a == 4 * BLOCK * D + 4 * D
    assert a - MP.maps_device_bytes(**dict(args, needs_movie=False)) == batch_buffer_bytes(4096, D, 2, True, 10)
    assert MP.maps_device_bytes(**dict(args, factors_on_device=True)) == a - 4 * 300 * 12
    assert MP.maps_device_bytes(**dict(args, factor_sums=True)) > a
    with pytest.raises(TypeError):
        MP.maps_device_bytes(*args.values())                       # keyword-only: no silent mis-ordering
    with pytest.raises(ValueError):
        MP.check_fit("regressor_maps", a, a - 1)
