"""Host side of localmd_amd.superpixels (no device): the float64 finish of the correlations against np.corrcoef, the
variance floor, non-finite sums, the edge bits at the image borders, relabelling and the size filter, the argument checks,
the memory plan, and tests/superpixel_ref.components against a brute-force flood fill."""
import importlib

import numpy as np
import pytest
import scipy.sparse

import localmd_amd
from localmd_amd.pmdarray import PMDArray
from tests import superpixel_ref as SR

SP = importlib.import_module("localmd_amd.superpixels")     # the module: localmd_amd.superpixels is the function


def _movie(T, d1, d2, seed):
    """A float32 movie whose neighbouring pixels share a signal, so correlations spread over (-1, 1)."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((T, d1 + 2, d2 + 2))
    X = base[:, 1:-1, 1:-1] + 0.7 * base[:, 2:, 1:-1] + 0.5 * base[:, 1:-1, 2:] - 0.4 * base[:, :-2, :-2]
    return (100.0 + 5.0 * X).astype(np.float32)


def test_finish_against_corrcoef_of_the_rectified_traces():
    T, d1, d2 = 400, 7, 9
    X = _movie(T, d1, d2, 1)
    thr = np.full((d1, d2), 100.0, np.float32)
    y = SR.rectified(X, thr)
    mom = SR.moments(y)
    rho = SP.finish_correlations(mom, T, d1, d2)
    assert rho.shape == (4, d1, d2) and rho.dtype == np.float64
    assert np.array_equal(rho, SR.finish(mom, T, d1, d2))
    y64 = y.astype(np.float64)
    worst = 0.0
    for b, (di, dj) in enumerate(SP.FORWARD):
        for i in range(d1):
            for j in range(d2):
                if 0 <= i + di < d1 and 0 <= j + dj < d2:
                    want = np.corrcoef(y64[:, i, j], y64[:, i + di, j + dj])[0, 1]
                    worst = max(worst, abs(rho[b, i, j] - want))
                else:
                    assert rho[b, i, j] == 0.0
    print("largest |rho - corrcoef|", worst)
    assert worst <= 1e-12
    assert np.abs(rho).max() > 0.5 and rho.min() < 0.0


def test_zero_variance_rule():
    """A constant y = 0 has var = 0 exactly.  A constant positive y has a var that is pure rounding of the two chains: it
    must fall below the floor 3 (T + 2) 2^-53 T S2 for every length, and a pixel one ulp-scale above constant must not."""
    for T in (3, 1000, 4097):
        for val in (0.1, 1.0 / 3.0, 1234.567):
            y = np.zeros((T, 2, 3), np.float32)
            y[:, 0, 0] = np.float32(val)                       # constant positive
            y[:, 0, 1] = np.float32(val)
            y[:, 1, 1] = np.float32(val) * (1.0 + 1e-3 * np.sin(np.arange(T)))   # alive, correlated with nothing
            y[:, 1, 2] = y[:, 1, 1]
            mom = SR.moments(y)
            S1, S2 = mom[0].reshape(2, 3), mom[1].reshape(2, 3)
            var = T * S2 - S1 * S1
            assert abs(var[0, 0]) <= SP.variance_floor(T) * T * S2[0, 0]
            assert var[1, 1] > SP.variance_floor(T) * T * S2[1, 1]
            rho = SP.finish_correlations(mom, T, 2, 3)
            assert np.array_equal(rho, SR.finish(mom, T, 2, 3))
            # every pair that touches a constant pixel is 0: E of (0,0) joins two constants, S of (0,1) a constant and a
            # live pixel; E of (1,1) joins two identical live pixels
            assert rho[0, 0, 0] == 0.0 and rho[2, 0, 1] == 0.0 and rho[3, 0, 0] == 0.0 and rho[1, 0, 2] == 0.0
            assert abs(rho[0, 1, 1] - 1.0) <= 1e-9
            assert not SP.edge_bytes(rho, 0.0)[0].any()        # rho = 0: no cut-off from 0 on joins a constant pixel
    assert SP.variance_floor(1000) == 3.0 * 1002 * 2.0 ** -53


def test_non_finite_sums_make_no_edge():
    T, d1, d2 = 50, 3, 3
    y = SR.rectified(_movie(T, d1, d2, 2), np.full((d1, d2), 99.0, np.float32))
    mom = SR.moments(y)
    clean = SP.edge_bytes(SP.finish_correlations(mom, T, d1, d2), -1.0)
    assert clean[0, 0] == 0b1101 and clean[1, 1] == 0b1111             # every in-image pair is an edge at cut_off -1
    bad = mom.copy().reshape(6, d1, d2)
    bad[0, 1, 1] = np.nan                   # S1 of the centre
    bad[0, 0, 0] = bad[1, 0, 0] = np.inf    # S1 and S2 of a corner, as an infinite value leaves them
    rho = SP.finish_correlations(bad, T, d1, d2)
    assert np.isnan(rho[0, 1, 1]) and not np.isfinite(rho[0, 0, 0])
    e = SP.edge_bytes(rho, -1.0)
    assert e[1, 1] == 0 and e[0, 0] == 0
    assert not (e[0, 1] & 0b0100) and not (e[0, 2] & 0b0010) and not (e[1, 0] & 0b0001)   # S, SW, E into the centre
    assert e[1, 2] == clean[1, 2] and e[2, 0] == clean[2, 0]
    assert np.array_equal(e, SR.edge_byte(rho, -1.0))
    c = SP.correlation_image(rho)
    assert np.all(np.isfinite(c)) and c.dtype == np.float32 and np.array_equal(c, SR.correlation(rho))
    inf_rho = np.zeros((4, 2, 2))
    inf_rho[0, 0, 0] = np.inf
    assert not SP.edge_bytes(inf_rho, 0.5).any()


def test_edge_bits_at_the_borders_and_the_correlation_image():
    d1, d2 = 4, 5
    mom = SR.moments(SR.rectified(_movie(60, d1, d2, 3), np.full((d1, d2), 95.0, np.float32)))
    rho = SP.finish_correlations(mom, 60, d1, d2)
    e = SP.edge_bytes(rho, -1.0)
    want = np.full((d1, d2), 0b1111, np.uint8)
    want[:, -1] &= 0b0110                   # last column: no E, no SE
    want[:, 0] &= 0b1101                    # first column: no SW
    want[-1, :] &= 0b0001                   # last row: E only
    assert np.array_equal(e, want)
    e9 = SP.edge_bytes(rho, 0.3)
    for b in range(4):
        assert np.array_equal((e9 >> b) & 1, rho[b] > 0.3)
    c = SP.correlation_image(rho)
    assert np.array_equal(c, SR.correlation(rho))
    assert c[0, 0] == np.float32(max(0.0, rho[0, 0, 0], rho[2, 0, 0], rho[3, 0, 0]))
    assert c[1, 1] == np.float32(max(0.0, rho[0, 1, 1], rho[1, 1, 1], rho[2, 1, 1], rho[3, 1, 1], rho[0, 1, 0], rho[1, 0, 2],
                                     rho[2, 0, 1], rho[3, 0, 0]))
    thr = SP.threshold_image(np.float32([[1.0, 2.0]]), np.float32([[0.1, 0.3]]), 2.0)
    assert thr.dtype == np.float32 and thr.shape == (1, 2)
    assert thr[0, 0] == np.float32(np.float32(2) * np.float32(0.1)) + np.float32(1)
    assert thr[0, 1] == np.float32(np.float32(2) * np.float32(0.3)) + np.float32(2)


def test_relabel_order_and_size_filter():
    root = np.array([[0, 0, 2, 3],
                     [0, 5, 2, 3],
                     [8, 5, 2, 3],
                     [8, 8, 8, 3]], np.int32)
    labels, sizes, n = SP.relabel(root, 1)
    assert n == 5 and labels.dtype == np.int32 and sizes.dtype == np.int64
    assert np.array_equal(sizes, [3, 3, 4, 2, 4])
    assert np.array_equal(labels, [[1, 1, 2, 3], [1, 4, 2, 3], [5, 4, 2, 3], [5, 5, 5, 3]])
    labels, sizes, n = SP.relabel(root, 3)
    assert n == 5 and np.array_equal(sizes, [3, 3, 4, 4])
    assert np.array_equal(labels, [[1, 1, 2, 3], [1, 0, 2, 3], [4, 0, 2, 3], [4, 4, 4, 3]])
    labels, sizes, n = SP.relabel(root, 3, 3)
    assert np.array_equal(sizes, [3, 3]) and np.array_equal(np.unique(labels), [0, 1, 2]) and labels[0, 2] == 2
    labels, sizes, n = SP.relabel(root, 5)
    assert n == 5 and sizes.shape == (0,) and not labels.any()
    for args in ((1,), (3,), (3, 3), (2, 3)):
        a, b = SP.relabel(root, *args), SR.number(root, *args)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), args


def _pmd(T=30, d1=6, d2=5):
    rng = np.random.default_rng(0)
    u = scipy.sparse.csr_matrix(rng.standard_normal((d1 * d2, 3)).astype(np.float32))
    return PMDArray(u, np.eye(3, dtype=np.float32), np.ones(3, np.float32), rng.standard_normal((3, T)).astype(np.float32),
                    (T, d1, d2), "C", np.zeros((d1, d2), np.float32), np.ones((d1, d2), np.float32))


class _Untouchable:
    dtype = np.dtype(np.float32)

    def __init__(self, shape):
        self.shape = shape

    def __getitem__(self, key):
        raise AssertionError("the movie was read")


def test_argument_checks_come_before_any_device_work():
    """None of these reaches the device: the machine that runs this test has none, and a device call would raise
    PMDLibraryError instead."""
    pmd = _pmd()
    mov = _Untouchable((30, 6, 5))
    bad = [dict(kind="residual"), dict(kind=("denoised",)), dict(th=np.nan), dict(th=np.inf), dict(th="2"),
           dict(cut_off=1.0), dict(cut_off=-1.5), dict(cut_off=np.nan), dict(min_size=0), dict(min_size=2.5),
           dict(min_size=True), dict(min_size=10, max_size=9), dict(max_size=2.0), dict(threshold=np.zeros((5, 6))),
           dict(threshold=np.zeros(30)), dict(threshold=np.zeros((6, 5), complex)), dict(kind="raw", movie=None)]
    for kw in bad:
        movie = kw.pop("movie", mov)
        with pytest.raises(ValueError):
            localmd_amd.superpixels(pmd, movie, **kw)
    with pytest.raises(ValueError, match="shape"):
        localmd_amd.superpixels(pmd, _Untouchable((30, 5, 6)), kind="raw")
    with pytest.raises(ValueError, match="no frames"):
        localmd_amd.superpixels(_pmd(T=0))
    with pytest.raises(ValueError, match="no frames"):
        pmd0 = _pmd(T=0)
        pmd0.superpixels(_Untouchable((0, 6, 5)), kind="raw")
    with pytest.raises(TypeError):
        localmd_amd.superpixels(np.zeros((3, 4, 5)))
    assert "superpixels" in localmd_amd.__all__ and "Superpixels" in localmd_amd.__all__


def test_memory_plan_and_read_counts():
    kw = dict(D=512 * 512, nb=10000, esize=2, n_cols=5000, rank=40, n_entries=9000, n_a=3_000_000, n_patches=4096,
              host_source=True, n_batches=3, factors_on_device=False)
    for kind in SP.KINDS:
        for given in (False, True):
            a = SP.superpixel_device_bytes(T=10_000, kind=kind, threshold_given=given, **kw)
            b = SP.superpixel_device_bytes(T=1_000_000, kind=kind, threshold_given=given, **kw)
            assert a == b, (kind, given)                            # no term grows with the movie's length
    D = kw["D"]
    own = SP.superpixel_device_bytes(T=10_001, kind="raw", threshold_given=True, **kw)
    assert own == 57 * D + 256 + 2 * 10000 * D * 2 + (1 << 20)
    sel = SP.superpixel_device_bytes(T=10_001, kind="raw", threshold_given=False, **kw)
    from localmd_amd.quantiles import quantile_device_bytes
    q = quantile_device_bytes(D=D, nb=10000, esize=2, n_raw=1, n_expand=0, n_pos=1, centred=True, n_cols=5000, rank=40,
                              n_entries=9000, n_a=3_000_000, n_patches=4096, needs_movie=True, host_source=True,
                              n_batches=3, factors_on_device=False)
    assert sel == max(own, q)
    two = SP.superpixel_device_bytes(T=10_000, kind="denoised", threshold_given=False, **kw)
    one = SP.superpixel_device_bytes(T=10_001, kind="denoised", threshold_given=False, **kw)
    assert two > one                                                # an even length needs two ranks for the median
    den = SP.superpixel_device_bytes(T=10_000, kind="denoised", threshold_given=True, **kw)
    assert den >= 57 * D + 4 * 1024 * D                             # the sums and one expanded block
    assert SP.movie_reads(4, "denoised") == 9 and SP.movie_reads(4, "raw") == 9 and SP.movie_reads(2, "raw") == 8
    assert SP.movie_reads(2, "raw", threshold_given=True) == 1 and SP.movie_reads(4, "denoised", True) == 1


def _flood(edges, d1, d2):
    e = np.asarray(edges).reshape(d1, d2)
    adj = {(i, j): [] for i in range(d1) for j in range(d2)}
    for i in range(d1):
        for j in range(d2):
            for b, (di, dj) in enumerate(SR.FORWARD):
                if (e[i, j] >> b) & 1 and 0 <= i + di < d1 and 0 <= j + dj < d2:
                    adj[i, j].append((i + di, j + dj))
                    adj[i + di, j + dj].append((i, j))
    root = -np.ones((d1, d2), np.int32)
    for i in range(d1):
        for j in range(d2):
            if root[i, j] >= 0:
                continue
            root[i, j] = i * d2 + j                                 # the first pixel met in index order is the smallest
            stack = [(i, j)]
            while stack:
                for q in adj[stack.pop()]:
                    if root[q] < 0:
                        root[q] = i * d2 + j
                        stack.append(q)
    return root


def test_reference_components_against_a_flood_fill():
    rng = np.random.default_rng(5)
    for d1, d2 in ((1, 1), (1, 9), (9, 1), (5, 7), (8, 8)):
        for density in (0.0, 0.1, 0.3, 0.6, 1.0):
            edges = np.zeros((d1, d2), np.uint8)
            for b in range(4):
                edges |= (rng.random((d1, d2)) < density).astype(np.uint8) << np.uint8(b)
            assert np.array_equal(SR.components(edges, d1, d2), _flood(edges, d1, d2)), (d1, d2, density)
    cross = np.zeros((2, 2), np.uint8)
    cross[0, 0], cross[0, 1] = 0b1000, 0b0010                       # SE of (0,0) and SW of (0,1) cross without meeting
    assert np.array_equal(SR.components(cross, 2, 2), [[0, 1], [1, 0]])
