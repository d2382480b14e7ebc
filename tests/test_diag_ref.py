"""tests/diag_ref.py is not trusted by fiat: its moments pushed through its image formulas reproduce the four routines of
oracle/diag_oracle.py (the restatement of the original's per-pixel loops), and the 35 fused moments are the moments of the
separate routines."""
import numpy as np
import pytest

from oracle import diag_oracle as DO
from tests import diag_ref as R

T, D1, D2 = 300, 7, 9
MODES = {"max": 0, "mean": 1}


def _case():
    """A float movie (a rank-3 signal on a mean image, plus noise) and a rank-3 stand-in for its decomposition."""
    rng = np.random.default_rng(11)
    space = rng.standard_normal((3, D1 * D2))
    time = np.cumsum(rng.standard_normal((T, 3)), axis=0)
    signal = (time @ space).reshape(T, D1, D2)
    movie = 50.0 + 5.0 * rng.random((D1, D2))[None] + signal + 2.0 * rng.standard_normal((T, D1, D2))
    stand_in = 50.0 + signal + 0.1 * rng.standard_normal((T, D1, D2))
    return movie, stand_in


@pytest.mark.parametrize("mode", ["max", "mean"])
def test_neighbour_images_reproduce_the_oracle(mode):
    y, x = _case()
    my, exists = R.neighbour_moments(y)
    mx, _ = R.neighbour_moments(x)
    mr, _ = R.neighbour_moments(y, x)
    assert my.shape == (10, D1 * D2) and exists.shape == (8, D1 * D2)
    assert exists[:, 0].sum() == 3 and exists[:, D2 + 1].sum() == 8      # a corner and an interior pixel
    m = MODES[mode]
    got = {"correlation": R.neighbour_image(my, None, T, D1, D2, 0, m),
           "pmd_correlation": R.neighbour_image(mx, my, T, D1, D2, 1, m),
           "residual_correlation": R.neighbour_image(mr, my, T, D1, D2, 1, m)}
    want = {"correlation": DO.make_correlation_image(y, mode), "pmd_correlation": DO.make_pmd_correlation_image(y, x, mode),
            "residual_correlation": DO.make_residual_correlation_image(y, x, mode)}
    for name in got:
        np.testing.assert_allclose(got[name].reshape(D1, D2), want[name], rtol=1e-10, atol=0, err_msg=name)


@pytest.mark.parametrize("lag", [1, 4])
def test_lag_image_reproduces_the_oracle(lag):
    y, _ = _case()
    mom = R.lag_moments(y, None, lag)
    assert mom.shape == (5, D1 * D2)
    np.testing.assert_allclose(R.lag_image(mom, T - lag).reshape(D1, D2), DO.make_autocorrelation_image(y, lag), rtol=1e-10,
                               atol=0)


@pytest.mark.parametrize("mode", ["max", "mean"])
def test_dead_pixels_follow_pythons_max(mode):
    """Zero-variance pixels at a corner, an edge and the interior: NaN where the oracle's loops (Python's ``max``) leave
    NaN, the same finite values elsewhere.  A dead pixel that is the last neighbour leaves NaN in the maximum; an earlier
    one is replaced by the next neighbour, without the floor at 0."""
    y, _ = _case()
    y = y.copy()
    for i, j in ((0, 0), (0, 4), (3, 5)):
        y[:, i, j] = 50.0
    got = R.neighbour_image(R.neighbour_moments(y)[0], None, T, D1, D2, 0, MODES[mode]).reshape(D1, D2)
    with np.errstate(all="ignore"):
        want = DO.make_correlation_image(y, mode)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=0, equal_nan=True)
    assert np.isnan(got[2, 4]) and np.isnan(got[3, 5])          # (3, 5) is the last neighbour of (2, 4)
    assert np.isnan(got[4, 6]) == (mode == "mean")              # and the first of (4, 6)


def test_shift_does_not_change_the_images():
    """Covariances are shift invariant: another reference frame gives the same image (to rounding)."""
    y, _ = _case()
    a = R.neighbour_image(R.neighbour_moments(y)[0], None, T, D1, D2, 0, 1)
    b = R.neighbour_image(R.neighbour_moments(y, ref=y[17])[0], None, T, D1, D2, 0, 1)
    np.testing.assert_allclose(a, b, rtol=1e-10, atol=0)


@pytest.mark.parametrize("lag", [1, 4])
def test_fused_moments_are_the_separate_moments(lag):
    rng = np.random.default_rng(5)
    mean = rng.integers(900, 1101, (D1, D2))
    y = mean[None] + rng.integers(-100, 101, (T, D1, D2))
    w = rng.integers(-60, 61, (T, D1, D2))
    mom, fss = R.fused_moments(y, w, mean, lag)
    assert mom.dtype == np.int64 and mom.shape == (35, D1 * D2) and fss.dtype == np.int64 and fss.shape == (T,)
    np.testing.assert_array_equal(mom[0:10], R.neighbour_moments(y)[0])
    np.testing.assert_array_equal(mom[10:20], R.neighbour_moments(w)[0])
    np.testing.assert_array_equal(mom[20:30], R.neighbour_moments(y - mean[None], w)[0])
    np.testing.assert_array_equal(mom[30:35], R.lag_moments(y, None, lag))
    np.testing.assert_array_equal(fss, ((y - mean[None] - w) ** 2).sum(axis=(1, 2)))


def test_degenerate_fields_of_view():
    """1 x 1: no neighbour exists, every clamped neighbour is the pixel itself; the mean image is 0 / 0, the maximum 0."""
    x = np.arange(12, dtype=np.int64).reshape(12, 1, 1) ** 2
    mom, exists = R.neighbour_moments(x)
    assert not exists.any()
    np.testing.assert_array_equal(mom[2:], np.repeat(mom[1:2], 8, axis=0))
    assert np.isnan(R.neighbour_image(mom, None, 12, 1, 1, 0, 1)).all()
    np.testing.assert_array_equal(R.neighbour_image(mom, None, 12, 1, 1, 0, 0), [0.0])


def test_expansion_references():
    import scipy.sparse

    rng = np.random.default_rng(2)
    u = scipy.sparse.random(12, 5, density=0.4, random_state=3, format="csr")
    u.data[:] = rng.integers(-8, 9, u.nnz)
    b = rng.integers(-8, 9, (5, 7))
    rows = np.array([3, 3, 0, 11])
    got = R.csr_rows_spmm(u.indptr, u.indices, u.data.astype(np.int64), rows, b, 6)
    np.testing.assert_array_equal(got, (u.toarray().astype(np.int64) @ b)[rows, :6])
    src, scale, shift = rng.integers(-9, 9, (4, 3)), np.array([1, 2, 4, 8]), np.array([0, -1, 5, 2])
    np.testing.assert_array_equal(R.transpose_affine(src, scale, shift), (src * scale[:, None] + shift[:, None]).T)
    np.testing.assert_array_equal(R.transpose_affine(src), src.T)
