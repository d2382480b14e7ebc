"""CPU checks of tests/eig_ref.py: the input builders and metrics of the eigensolver tests are exercised on
numpy.linalg.eigh in float64, rounded to fp32 - the best an fp32-output solver can return.  Every bound the GPU tests
(tests/test_gpu_eigensolver.py) assert is met by that reference alone: the conditions are satisfiable."""
import numpy as np
import pytest

from tests import eig_ref as R

ORDERS = (66, 600)


@pytest.fixture(scope="module")
def rounded_reference():
    cache = {}

    def get(kind, n):
        if (kind, n) not in cache:
            S = R.make_sym(kind, n, seed=n)
            w64, V = R.reference_eigh(S)
            cache[kind, n] = (S, w64, V, R.floor_null(w64), V.T.astype(np.float32))
        return cache[kind, n]

    return get


@pytest.mark.parametrize("n", ORDERS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_builders_are_exactly_symmetric_float32(kind, n):
    S = R.make_sym(kind, n, seed=n)
    assert S.dtype == np.float32 and S.shape == (n, n)
    assert np.array_equal(S, S.T) and np.all(np.isfinite(S))
    assert np.array_equal(S, R.make_sym(kind, n, seed=n))


@pytest.mark.parametrize("n", ORDERS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_rounded_reference_meets_every_gpu_bound(rounded_reference, kind, n):
    S, w64, V, w, E = rounded_reference(kind, n)
    b = R.route_bounds(S)
    assert R.is_ascending(w)
    assert R.eig_abs_err(w, w64) <= b["eig"]
    orth, res = R.orth_err(E), R.resid(E, S, w)
    assert orth <= b["orth"] and res <= b["resid"]
    lmax = float(np.abs(w64).max())
    for sin, bound in R.group_sin_theta(E, S, 1e-3 * lmax, w, ref=(w64, V)):
        assert sin <= bound + orth
    if kind == "zero":
        assert np.all(w == 0)
    if kind in R.LOW_RANK_KINDS:
        aw = np.abs(w.astype(np.float64))
        assert np.all((aw == 0) | (aw >= R.EPS32 * float(aw.max()) * (1 - 2.0 ** -23)))


def test_rank_of_the_low_rank_kinds():
    n = 600
    wg = np.linalg.eigvalsh(R.make_sym("gram_lowrank", n, 1).astype(np.float64))
    assert np.count_nonzero(np.abs(wg) > 1e-5 * wg.max()) == n // 15   # the rest is the rounding of the fp32 product
    assert np.linalg.matrix_rank(R.make_sym("zero_tail", n, 1).astype(np.float64)) == n // 3
    assert not R.make_sym("zero", n, 1).any()
    odd = R.make_sym("indefinite", 67, 1)
    assert not odd[-1].any() and not odd[:, -1].any()
    D = R.make_sym("diagonal", 66, 1)
    assert np.array_equal(D, np.diag(np.diag(D)))
    T = R.make_sym("tridiagonal", 66, 1)
    assert not np.triu(T, 2).any() and np.triu(T, 1).any()


def test_spectral_groups_and_sin_theta_on_a_known_rotation():
    """Two eigenvalues 1e-6 apart and one far away: a rotation inside the pair costs nothing, a rotation out of it is seen
    in full and stays under the Davis-Kahan bound."""
    S = np.diag([1.0, 1.0 + 1e-6, 3.0])
    assert R.spectral_groups([1.0, 1.0 + 1e-6, 3.0], 1e-3) == [(0, 2), (2, 3)]
    c, s = np.cos(0.3), np.sin(0.3)
    inside = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1.0]])
    w = np.array([1.0, 1.0 + 1e-6, 3.0])
    for sin, _ in R.group_sin_theta(inside, S, 1e-3, w):
        assert sin < 1e-12
    t = 1e-4
    out = np.array([[1, 0, 0], [0, np.cos(t), np.sin(t)], [0, -np.sin(t), np.cos(t)]])
    got = R.group_sin_theta(out, S, 1e-3, w)
    assert abs(got[0][0] - np.sin(t)) < 1e-12 and abs(got[1][0] - np.sin(t)) < 1e-12
    assert all(sin <= bound for sin, bound in got)


@pytest.fixture(scope="module")
def fp32_solver():
    from scipy.linalg import eigh

    def solve(S):
        w0, V0 = eigh(S, driver="evd")
        assert w0.dtype == np.float32
        return w0, np.ascontiguousarray(V0.T)

    return solve


@pytest.mark.parametrize("kind", ["separated", "repeated", "cluster", "gram_lowrank", "graded"])
def test_refinement_restatement_and_its_ordering(fp32_solver, kind):
    """The Rayleigh quotients of the refined vectors of an fp32 divide-and-conquer solver (LAPACK ssyevd here) leave the
    refinement out of order inside clusters and null spaces; ranked, they ascend and the vectors follow."""
    n = 600
    S = R.make_sym(kind, n, seed=n)
    w0, E0 = fp32_solver(S)
    w_raw, E_raw = R.refine_reference(S, w0, E0, ordered=False)
    w, E = R.refine_reference(S, w0, E0)
    if kind == "separated":
        assert R.is_ascending(w_raw)
        assert np.array_equal(w, w_raw) and np.array_equal(E, E_raw)
        # the refinement is what the tight bounds of the GPU tests see: fp32 solver against refined, on the same matrix
        w64, V = R.reference_eigh(S)
        Er = V.T.astype(np.float32)
        assert R.orth_err(E) <= 4 * R.orth_err(Er) + 1e-7
        smax = float(np.abs(S).max())
        assert R.resid(E, S, w) / smax <= 4 * R.resid(Er, S, R.floor_null(w64)) / smax + 1e-7
        assert R.orth_err(E0) > 4 * R.orth_err(Er) + 1e-7
    else:
        assert not R.is_ascending(w_raw)
    assert R.is_ascending(w)
    assert np.array_equal(np.sort(w_raw), w)   # the same values, and each vector stays with its value
    b = R.route_bounds(S)
    assert R.orth_err(E) <= b["orth"] and R.resid(E, S, w) <= b["resid"]


def test_householder_q_matches_lapack():
    from scipy.linalg import lapack

    n = 23
    S = R.make_sym("separated", n, seed=5)
    # column-major lower triangle of LAPACK = the memory-upper triangle of the library's row-major buffer
    c, d, e, tau, info = lapack.ssytrd(S, lower=1)
    assert info == 0
    # sorgtr('L') = the identity in the first row and column around sorgqr of the reflectors shifted up by one
    # (SciPy wraps sorgqr only)
    q1, _, info = lapack.sorgqr(np.asfortranarray(c[1:, :n - 1]), tau)
    assert info == 0
    q = np.eye(n, dtype=np.float32)
    q[1:, 1:] = q1
    Q = R.householder_q(np.ascontiguousarray(c.T), tau)
    assert np.abs(Q - q).max() < 5e-6
    Tm = np.diag(d.astype(np.float64)) + np.diag(e.astype(np.float64), 1) + np.diag(e.astype(np.float64), -1)
    assert np.abs(Q.T @ S.astype(np.float64) @ Q - Tm).max() < 3e-6 * np.abs(S).max() * np.sqrt(n)
