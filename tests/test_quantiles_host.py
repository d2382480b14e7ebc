"""Host side of localmd_amd.quantile_images (no GPU): the order-preserving keys and their inverse, a NumPy emulation of
the four digit passes of csrc/quantile.hip against np.sort, the positions against np.quantile, the float64 finish,
argument errors before any device work and before the movie is read, and a device-memory plan that does not depend on the
movie's length."""
import numpy as np
import pytest

import localmd_amd
from localmd_amd import quantiles as QT
from localmd_amd._stream import block_plan
from localmd_amd.pmdarray import PMDArray
from tests.test_traces_host import _Untouchable, _pmd, no_device  # noqa: F401 - no_device is a fixture

T, D1, D2 = 300, 6, 7
LENGTHS = (1, 2, 7, 257, 1030)
QS = (0.0, 0.08, 0.5, 0.9, 1.0)


def test_reexported():
    assert localmd_amd.quantile_images is QT.quantile_images
    assert "quantile_images" in localmd_amd.__all__
    assert callable(PMDArray.quantiles)
    assert QT.INTERPOLATIONS == ("linear", "lower", "higher", "nearest") and QT.MAD_TO_STD == 1.4826


def test_result_object():
    img = np.zeros((2, D1, D2), np.float32)
    r = QT.Quantiles(raw=img, q=(0.08, 0.5), interpolation="lower")
    assert r.denoised is None and r.residual is None and r.mad is None and r.raw is img
    assert r.q == (0.08, 0.5) and r.interpolation == "lower"
    assert repr(r) == "Quantiles(raw; q=(0.08, 0.5); lower)"


# ---- keys ----------------------------------------------------------------------------------------------------------
def _edge_values():
    tiny = np.float32(1e-45)                                     # the smallest denormal
    one = np.float32(1.0)
    fmax = np.finfo(np.float32).max
    return np.array([-np.inf, -fmax, -2.0, np.nextafter(-one, np.float32(-2)), -one, np.nextafter(-one, np.float32(0)),
                     -np.finfo(np.float32).tiny, -2 * tiny, -tiny, -0.0, 0.0, tiny, 2 * tiny, np.finfo(np.float32).tiny,
                     np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(2)), 2.0, 65535.0, fmax, np.inf],
                    dtype=np.float32)


def test_keys_order_and_round_trip():
    x = _edge_values()
    assert np.all(x[:-1] <= x[1:]) and x[1] < 0 and x[8] == -x[11] and x[8] != 0       # denormals survive
    k = QT.float_keys(x)
    assert k.dtype == np.uint32
    assert np.all(k[:-1] < k[1:])                         # strictly increasing: -0 before +0, adjacent floats apart
    assert k[10] == 0x80000000 and k[9] == 0x7FFFFFFF     # +0 and -0
    assert k[16] - k[15] == 1 and k[15] - k[14] == 1 and k[5] - k[4] == 1      # neighbours of +-1 are neighbouring keys
    back = QT.key_floats(k)
    assert back.dtype == np.float32 and back.tobytes() == x.tobytes()
    nans = np.array([np.nan, -np.nan, np.float32(np.nan)], np.float32)
    nans = np.concatenate([nans, np.array([0x7FC00001, 0xFFFFFFFF, 0x7F800001], np.uint32).view(np.float32)])
    kn = QT.float_keys(nans)
    assert np.all(kn == 0xFFFFFFFF) and kn.max() > k.max()                    # every NaN is the largest key
    assert np.all(np.isnan(QT.key_floats(kn)))
    rng = np.random.default_rng(0)
    r = rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    r = r[~np.isnan(r)]
    assert QT.key_floats(QT.float_keys(r)).tobytes() == r.tobytes()
    order = np.argsort(QT.float_keys(r), kind="stable")
    assert np.array_equal(r[order], np.sort(r))
    # integers in 16-bit containers: the float has its low 8 bits zero, so the key's last digit is 0x00, or 0xFF when negative
    i16 = np.arange(-32768, 32768).astype(np.float32)
    k16 = QT.float_keys(i16)
    assert np.all((k16 & 0xFF) == np.where(i16 < 0, 0xFF, 0))
    assert np.all(((k16 >> 8) & 0x800000 != 0) == (i16 >= 0))
    assert np.all((QT.float_keys(np.arange(65536).astype(np.float32)) & 0xFF) == 0)


# ---- the digit passes, emulated --------------------------------------------------------------------------------------
def emulate_select(keys, rank, passes=4):
    """The prefix pmd_pixel_hist_accumulate / pmd_pixel_hist_select leave after ``passes`` passes (include/pmd_hip.h) for
    the (n, N) uint32 keys and the rank: per pass the 256 counts of digit (key >> (24 - 8 p)) & 255 among the elements with
    key >> (32 - 8 p) == prefix, the first bin whose cumulative count exceeds the rank, rank -= the count below it,
    prefix = prefix << 8 | bin."""
    keys = np.asarray(keys, np.uint32).astype(np.uint64)
    n, N = keys.shape
    prefix = np.zeros(N, np.uint64)
    rank = np.full(N, rank, np.int64)
    for p in range(passes):
        for c in range(N):
            k = keys[:, c]
            use = np.ones(n, bool) if p == 0 else (k >> np.uint64(32 - 8 * p)) == prefix[c]
            hist = np.bincount(((k[use] >> np.uint64(24 - 8 * p)) & np.uint64(255)).astype(np.int64), minlength=256)
            cum = np.cumsum(hist)
            b = int(np.argmax(cum > rank[c]))
            assert cum[b] > rank[c]
            rank[c] -= cum[b] - hist[b]
            prefix[c] = (prefix[c] << np.uint64(8)) | np.uint64(b)
    return prefix.astype(np.uint32), rank


def _columns(n, rng):
    one = np.float32(1.0)
    near = np.array([np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(2))], np.float32)
    cols = [rng.integers(0, 7, n).astype(np.float32),                                   # ties everywhere
            np.full(n, 900.0, np.float32),                                              # constant
            -rng.integers(0, 7, n).astype(np.float32) - 1.0,                            # negated
            (900.0 + 8.0 * rng.standard_normal(n)).astype(np.float32),
            near[rng.integers(0, 3, n)],                                                # keys that differ in the last digit
            rng.choice(np.array([-3.5, 3.5], np.float32), n),                           # ... only in the sign
            rng.choice(np.array([-np.inf, -1.0, 2.0, np.inf], np.float32), n)]
    withnan = (rng.standard_normal(n)).astype(np.float32)
    withnan[n // 2] = np.nan
    cols.append(withnan)
    return np.stack(cols, axis=1)


def test_emulated_passes_select_the_order_statistic():
    rng = np.random.default_rng(1)
    for n in LENGTHS:
        y = _columns(n, rng)
        want = np.sort(y, axis=0)
        keys = QT.float_keys(y)
        for k in sorted({0, (n - 1) // 2, n // 2, n - 1, int(0.08 * (n - 1))}):
            prefix, left = emulate_select(keys, k)
            got = QT.key_floats(prefix)
            assert np.array_equal(got, want[k], equal_nan=True), (n, k)
            assert np.all(left >= 0)
        # 16-bit integers need three passes
        y16 = rng.integers(-300, 300, (n, 3)).astype(np.int16).astype(np.float32)
        p3, _ = emulate_select(QT.float_keys(y16), n // 2, passes=3)
        k3 = (p3 << np.uint32(8)) | np.where(p3 & np.uint32(0x800000), np.uint32(0), np.uint32(0xFF))
        assert np.array_equal(QT.key_floats(k3), np.sort(y16, axis=0)[n // 2]), n
    # NaN sorts last
    y = np.array([[np.nan], [1.0], [np.nan], [-2.0]], np.float32)
    assert QT.key_floats(emulate_select(QT.float_keys(y), 1)[0])[0] == 1.0
    assert np.isnan(QT.key_floats(emulate_select(QT.float_keys(y), 2)[0])[0])


# ---- positions and the finish ----------------------------------------------------------------------------------------
def test_positions_agree_with_numpy():
    for n in LENGTHS:
        y = 3.0 * np.arange(n, dtype=np.float64) - 7.0              # distinct, sorted: the value names its position
        h, lo, hi, near = QT.positions(QS, n)
        assert h.dtype == np.float64 and np.array_equal(h, np.asarray(QS) * (n - 1))
        for name, pos in (("lower", lo), ("higher", hi), ("nearest", near)):
            assert pos.min() >= 0 and pos.max() <= n - 1
            want = np.quantile(y, QS, method=name)
            assert y[pos].tobytes() == want.tobytes(), (n, name)
        assert lo[0] == hi[0] == 0 and lo[-1] == hi[-1] == n - 1
        assert np.all(hi - lo <= 1) and np.all((hi == lo) == (h == np.floor(h)))
    # half-way positions round to even
    assert list(QT.positions((0.5,), 2)[3]) == [0] and list(QT.positions((0.5,), 4)[3]) == [2]
    assert list(QT.positions((0.25, 0.75), 7)[3]) == [2, 4]         # h = 1.5, 4.5


def test_linear_finish():
    rng = np.random.default_rng(2)
    lo = (900.0 + 8.0 * rng.standard_normal(1000)).astype(np.float32)
    hi = (lo + np.abs(rng.standard_normal(1000))).astype(np.float32)
    for frac in (0.0, 0.32, 0.5, 0.999):
        got = QT.finish_linear(lo, hi, frac)
        want = (lo.astype(np.float64) + (hi.astype(np.float64) - lo.astype(np.float64)) * frac).astype(np.float32)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert QT.finish_linear(lo, hi, 0.0).tobytes() == lo.tobytes()
    # against NumPy on float64 data that is exact in float32: the same number up to the one rounding
    for n in LENGTHS:
        y = np.sort(rng.integers(0, 4000, n)).astype(np.float32)
        for qq in QS:
            (a, b, frac), = QT._needed((qq,), n, "linear")
            got = QT.finish_linear(y[a], y[b], frac)
            want = np.quantile(y.astype(np.float64), qq)
            assert abs(float(got) - want) <= 2.0 ** -23 * abs(want), (n, qq)
            for name in ("lower", "higher", "nearest"):
                (a, b, frac), = QT._needed((qq,), n, name)
                assert a == b and frac == 0.0 and y[a] == np.quantile(y, qq, method=name)


def test_check_q():
    assert QT.check_q(0.5) == (0.5,) and QT.check_q(1) == (1.0,) and QT.check_q(np.float32(0.25)) == (0.25,)
    assert QT.check_q([0.5, 0.0, 0.5]) == (0.5, 0.0, 0.5)          # duplicates, the caller's order
    assert QT.check_q(np.array([0.08, 1.0])) == (0.08, 1.0)
    for bad in (-0.1, 1.0001, np.nan, (), [0.5, 2], "0.5", None, True, [[0.5]], [0.5, "a"], 1j):
        with pytest.raises(ValueError):
            QT.check_q(bad)


def test_movie_passes():
    assert QT.movie_passes(2, "raw") == 3 and QT.movie_passes(4, "raw") == 4
    assert QT.movie_passes(2, ("raw", "denoised")) == 3 and QT.movie_passes(2, ("raw", "residual")) == 4
    assert QT.movie_passes(2, "raw", mad=True) == 7 and QT.movie_passes(4, ("denoised", "raw", "residual"), mad=True) == 8
    assert QT.movie_passes(2, "denoised", mad=True) == 0 and QT.movie_passes(4, ("denoised",)) == 0


# ---- argument errors -------------------------------------------------------------------------------------------------
def _bad_calls():
    mov = _Untouchable((T, D1, D2))
    return [
        dict(kinds="noise"),
        dict(kinds=()),
        dict(kinds=("raw", "raw"), movie=mov),
        dict(kinds=3),
        dict(q=-0.01),
        dict(q=1.5),
        dict(q=()),
        dict(q=float("nan")),
        dict(q="median"),
        dict(q=(0.5, None)),
        dict(q=True),
        dict(interpolation="midpoint"),
        dict(interpolation=None),
        dict(mad=1),
        dict(mad="yes"),
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
            localmd_amd.quantile_images(pmd, **kw)
        with pytest.raises(ValueError):
            pmd.quantiles(**kw)
    with pytest.raises(TypeError):
        localmd_amd.quantile_images(np.zeros((T, D1, D2)))
    empty = _pmd(0, D1, D2)
    with pytest.raises(ValueError, match="no frames"):
        localmd_amd.quantile_images(empty)
    with pytest.raises(ValueError, match="no frames"):
        empty.quantiles(_Untouchable((0, D1, D2)), kinds="raw", q=(0.0, 1.0), mad=True)


# ---- the memory plan -------------------------------------------------------------------------------------------------
def _plan_bytes(T, fbs, **kw):
    plan = block_plan(T, fbs)
    args = dict(D=4096, nb=plan[0][1] - plan[0][0], esize=2, n_raw=1, n_expand=2, n_pos=3, centred=False, n_cols=300,
                rank=12, n_entries=900, n_a=50000, n_patches=64, needs_movie=True, host_source=True,
                n_batches=len(plan), factors_on_device=False)
    args.update(kw)
    return QT.quantile_device_bytes(**args)


def test_device_bytes_do_not_grow_with_the_movie():
    from localmd_amd._stream import BLOCK, batch_buffer_bytes

    a = _plan_bytes(10 ** 4, 4096)
    assert a == _plan_bytes(10 ** 6, 4096)
    D = 4096
    # 1 KB of histogram and 8 bytes of rank and prefix per pixel, kind and rank
    assert _plan_bytes(10 ** 4, 4096, n_pos=4) - a == (1024 + 8) * 3 * D
    assert a - _plan_bytes(10 ** 4, 4096, n_raw=0) == 3 * (1024 + 8) * D
    assert _plan_bytes(10 ** 4, 4096, centred=True) - a == 4 * 3 * D
    assert a - _plan_bytes(10 ** 4, 4096, n_expand=1) == 3 * (1024 + 8) * D + 4 * BLOCK * D
    assert a - _plan_bytes(10 ** 4, 4096, needs_movie=False) == batch_buffer_bytes(4096, D, 2, True, 3)
    assert _plan_bytes(10 ** 4, 4096, factors_on_device=True) == a - 4 * 300 * 12
    # a last group of fewer than 64 pixels still holds a whole group of counters
    one = QT.quantile_device_bytes(D=65, nb=8, esize=4, n_raw=1, n_expand=0, n_pos=1, centred=False, n_cols=0, rank=0,
                                   n_entries=0, n_a=0, n_patches=0, needs_movie=False, host_source=True, n_batches=1,
                                   factors_on_device=False)
    assert one == 2 * 65536 + 8 * 65 + (1 << 20)
    with pytest.raises(TypeError):
        QT.quantile_device_bytes(4096, 4096, 2)                    # keyword-only: no silent mis-ordering
    with pytest.raises(ValueError):
        QT.check_fit("quantile_images", a, a - 1)
