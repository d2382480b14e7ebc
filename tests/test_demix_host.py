"""Host side of the demixing solver (localmd_amd/demix.py) and its NumPy statements (tests/hals_ref.py): the emulated sweep
against float64, the float64 reference on planted data, the end-of-call shift, the offset algebra against brute force on
the expanded movie, the pixel-major tables, argument checks and the memory plan.  No device needed."""
import importlib

import numpy as np
import pytest
import scipy.sparse

import localmd_amd
from localmd_amd import _lib
from localmd_amd.pmdarray import PMDArray
from localmd_amd.traces import denoised_factors, roi_weights
from tests import hals_ref as HR
from tests.test_export_host import _random_tiled_u
from tests.test_traces_host import _disc

DX = importlib.import_module("localmd_amd.demix")     # the module: localmd_amd.demix is the function it exports
U24 = 2.0 ** -24


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a device context fails the test: the checks must come first."""
    def refuse(*a, **k):
        raise AssertionError("a device context was opened before the argument checks")
    monkeypatch.setattr(_lib.Context, "__init__", refuse)


def _small_pmd(order, T=50, d1=12, d2=10, rank=5, seed=3):
    u = _random_tiled_u(d1, d2, 6, 5, order, 1, seed=seed)
    rng = np.random.default_rng(seed + 1)
    k = u.shape[1]
    return PMDArray(u, rng.standard_normal((k, rank)) * 0.3, np.linspace(9, 2, rank),
                    rng.standard_normal((rank, T)) * 0.2 + rng.uniform(-0.1, 0.1, (rank, 1)), (T, d1, d2), order,
                    rng.uniform(50, 150, (d1, d2)), rng.uniform(0.5, 3, (d1, d2)))


def _expand64(pmd):
    """The denoised movie as (D, T) float64 with pixels in C order."""
    T, d1, d2 = pmd.shape
    u_of_c = np.asarray(pmd.row_indices).reshape(-1)
    low = (pmd.u.astype(np.float64) @ (pmd.r.astype(np.float64) * pmd.s.astype(np.float64)[None, :])) @ pmd.v.astype(np.float64)
    return (np.asarray(pmd.mean_img, np.float64).reshape(-1)[:, None]
            + np.asarray(pmd.var_img, np.float64).reshape(-1)[:, None] * np.asarray(low)[u_of_c])


# ---- the sweep ------------------------------------------------------------------------------------------------------
def _dominant_g(K, rng, density=0.4):
    """A symmetric CSR G with the diagonal stored and G_kk = 2 sum_{j != k} |G_kj| (rho = 1/2), fp32-exact values."""
    off = np.triu((rng.random((K, K)) < density) * rng.uniform(-1, 1, (K, K)), 1)
    off = (off + off.T).astype(np.float32).astype(np.float64)
    G = off + np.diag((2.0 * np.abs(off).sum(axis=1) + 0.5).astype(np.float32).astype(np.float64))
    S = scipy.sparse.csr_matrix(G)
    S.sort_indices()
    return G, S


def test_emulated_sweep_against_float64_on_a_diagonally_dominant_system():
    """One update forms v = C_k + (P_k - sum_i g_i c_i) invd_k from m products, m subtractions, one product and one
    addition, each rounded once (u = 2^-24).  A term passes through at most m + 3 of those roundings (its own product,
    at most m subtractions, the step and the final addition), so to first order the update's own error is
    delta_k <= (m + 3) u (|C_k| + (|P_k| + sum_i |g_i c_i|) |invd_k|) = (m + 3) u sum|terms|, and 1.01 covers the
    second-order terms for m <= 70.  The errors e_j the rows j != k bring in are damped by
    rho = max_k sum_{j != k} |G_kj| / G_kk = 1/2 < 1 here, and max(lo, .) does not enlarge a difference, so
    e_k <= delta_k + rho max_j e_j and by induction over k every error stays below max_k delta_k / (1 - rho): the
    rounding errors do not accumulate beyond the per-update error.  invd is rounded to fp32 before both runs (the
    inputs are the same numbers), and the float64 run is the reference."""
    rng = np.random.default_rng(0)
    K, n = 40, 33
    G, S = _dominant_g(K, rng)
    rho = np.max((np.abs(G).sum(axis=1) - np.diag(G)) / np.diag(G))
    assert rho < 0.51
    C32 = rng.standard_normal((K, n)).astype(np.float32)
    P32 = (3 * rng.standard_normal((K, n))).astype(np.float32)
    invd32 = (1.0 / np.diag(G)).astype(np.float32)
    lo32 = np.where(np.arange(K) % 3 == 0, -np.inf, 0.0).astype(np.float32)
    C64 = C32.astype(np.float64)
    got = HR.hals_sweep(C32.copy(), P32, S.indptr, S.indices, S.data.astype(np.float32), invd32, lo32)
    assert got.dtype == np.float32
    # float64, keeping sum|terms| of every update
    delta = np.zeros((K, n))
    for k in range(K):
        i0, i1 = S.indptr[k], S.indptr[k + 1]
        terms = np.abs(P32[k].astype(np.float64))
        acc = P32[k].astype(np.float64)
        for i in range(i0, i1):
            prod = S.data[i] * C64[S.indices[i]]
            acc, terms = acc - prod, terms + np.abs(prod)
        m = i1 - i0
        delta[k] = 1.01 * (m + 3) * U24 * (np.abs(C64[k]) + terms * float(invd32[k]))
        C64[k] = np.maximum(float(lo32[k]), C64[k] + acc * float(invd32[k]))
    err = np.abs(got.astype(np.float64) - C64)
    bound = delta.max() / (1.0 - rho)
    assert err.max() > 0                      # the two runs do differ: the comparison is not vacuous
    assert err.max() <= bound, (err.max(), bound)
    assert np.all(got[lo32 == 0] >= 0) and got[lo32 != 0].min() < 0


def test_sweep_leaves_rows_with_zero_invd_untouched():
    rng = np.random.default_rng(1)
    G, S = _dominant_g(6, rng, density=0.8)
    C = rng.standard_normal((6, 9))
    invd = 1.0 / np.diag(G)
    invd[2] = 0.0
    out = HR.hals_sweep(C.copy(), rng.standard_normal((6, 9)), S.indptr, S.indices, S.data, invd, np.zeros(6))
    assert np.array_equal(out[2], C[2]) and not np.array_equal(out[3], C[3])


# ---- the float64 reference on planted data -------------------------------------------------------------------------
def _planted(seed=1, d1=12, d2=12, T=40):
    rng = np.random.default_rng(seed)
    masks = np.stack([_disc(d1, d2, 4, 4, 3.2), _disc(d1, d2, 6, 7, 3.2), _disc(d1, d2, 8, 4, 2.6)])
    assert (masks[0] & masks[1]).any() and (masks[1] & masks[2]).any() and (masks[0] & masks[2]).any()
    S = masks.reshape(3, -1).T
    A = S * rng.uniform(0.5, 1.5, S.shape)
    C = rng.exponential(1.0, (3, T)) * (rng.random((3, T)) < 0.4)
    b = rng.uniform(1, 2, d1 * d2)
    return A @ C + b[:, None], S


def test_reference_recovers_planted_data():
    """X = A* C* + b* without noise, from the true supports with flat weights.  J is non-increasing, and the residual
    ||X - A C - b||^2 falls by about a factor of ten per outer iteration: relative to ||X - mbar||^2 the float64 reference
    reaches 9.8e-4, 4.0e-5, 2.8e-6, 2.5e-7, 2.5e-8 and 2.7e-9 after iterations 1 .. 6.  The floor asked of the last one
    is 1e-8 (reached: 2.7e-9), and J, which is the residual minus the constant, must agree with it."""
    X, S = _planted()
    r = HR.demix_ref(X, S.astype(np.float64), S, outer_iters=6, sweeps=5)
    J, res = r["objective"], r["residual"]
    const = ((X - X.mean(axis=1, keepdims=True)) ** 2).sum()
    assert np.all(np.diff(J) <= 0) and np.all(np.diff(res) < 0)
    assert np.allclose(J + const, res, rtol=0, atol=1e-9 * const)
    assert res[-1] <= 1e-8 * const, res[-1] / const
    assert res[-1] < 1e-5 * res[0]
    rec = r["footprints"] @ r["traces"] + r["background"][:, None]
    assert np.abs(((rec - X) ** 2).sum() - res[-1]) <= 1e-9 * const      # A C + b after the shift is the same fit
    assert np.all(r["footprints"] >= 0) and np.all(r["footprints"][~S] == 0) and not r["empty"].any()


def test_end_of_call_shift():
    X, S = _planted(seed=2)
    r = HR.demix_ref(X, S.astype(np.float64), S, outer_iters=2, sweeps=3)
    A, C0 = r["footprints"], r["unshifted"]
    mbar = X.mean(axis=1)
    assert np.array_equal(r["traces"].min(axis=1), np.zeros(3))
    before = A @ C0 + (mbar - A @ C0.mean(axis=1))[:, None]
    after = A @ r["traces"] + r["background"][:, None]
    assert np.abs(before - after).max() <= 1e-12 * np.abs(before).max()
    # unbounded traces are not shifted
    r2 = HR.demix_ref(X, S.astype(np.float64), S, outer_iters=1, sweeps=2, nonneg_traces=False)
    assert np.array_equal(r2["traces"], r2["unshifted"]) and r2["traces"].min() < 0


# ---- the offset algebra and the tables of demix ---------------------------------------------------------------------
def _rois(d1, d2):
    return np.stack([_disc(d1, d2, 4, 3, 2.5), _disc(d1, d2, 6, 5, 2.5), _disc(d1, d2, 9, 7, 1.5), np.ones((d1, d2), bool)])


@pytest.mark.parametrize("order", ["C", "F"])
def test_offsets_and_time_mean_against_the_expanded_movie(order):
    pmd = _small_pmd(order)
    T, d1, d2 = pmd.shape
    X = _expand64(pmd)
    W, _ = roi_weights(_rois(d1, d2) * np.random.default_rng(0).uniform(0.5, 2, (4, d1, d2)), (d1, d2), order, "sum")
    A = scipy.sparse.csr_matrix((DX.unit_columns(W), W.indices, W.indptr), shape=W.shape)
    assert np.allclose(np.asarray(A.multiply(A).sum(axis=1)).reshape(-1), 1.0, rtol=1e-14)
    qv, mbar = DX.time_mean_factors(pmd)
    assert np.abs(mbar - X.mean(axis=1)).max() <= 1e-12 * np.abs(X).max()
    B, off = denoised_factors(pmd, A)
    G, invd = DX.gram(A, np.zeros(4, dtype=bool))
    assert np.allclose(G.toarray(), (A @ A.T).toarray()) and np.allclose(invd * G.diagonal(), 1.0)
    assert np.all(np.diff(G.indptr) >= 1) and all(k in G.indices[G.indptr[k]:G.indptr[k + 1]] for k in range(4))
    cbar = np.random.default_rng(1).uniform(0, 2, 4)
    Q = pmd.r.astype(np.float64) * pmd.s.astype(np.float64)[None, :]
    P = np.asarray(B @ Q) @ pmd.v.astype(np.float64) + DX.sweep_offsets(B, G, qv, cbar)[:, None]
    brute = A @ (X - mbar[:, None]) + (G @ cbar)[:, None]
    assert np.abs(P - brute).max() <= 1e-11 * np.abs(brute).max()


def test_cover_tables_are_the_pixel_major_view():
    d1, d2 = 12, 10
    W, _ = roi_weights(_rois(d1, d2) * np.random.default_rng(2).uniform(0.5, 2, (4, d1, d2)), (d1, d2), "C", "sum")
    t = DX.cover_tables(W)
    dense = W.toarray()
    assert np.array_equal(t["px"], np.nonzero((dense != 0).any(axis=0))[0])
    assert t["cov_ptr"][0] == 0 and t["cov_ptr"][-1] == W.nnz == len(t["cov_k"]) == len(t["perm"])
    assert np.array_equal(np.sort(t["perm"]), np.arange(W.nnz))
    for q, p in enumerate(t["px"]):
        j0, j1 = t["cov_ptr"][q], t["cov_ptr"][q + 1]
        ks = t["cov_k"][j0:j1]
        assert np.array_equal(ks, np.nonzero(dense[:, p])[0])
        assert np.array_equal(W.data[t["perm"][j0:j1]], dense[ks, p])


def test_pixel_statement_matches_the_dense_reference_step():
    """hals_pixels on the factors gives what the dense spatial step of demix_ref does on the expanded movie."""
    pmd = _small_pmd("F")
    T, d1, d2 = pmd.shape
    X = _expand64(pmd)
    W, _ = roi_weights(_rois(d1, d2), (d1, d2), "F", "sum")
    t = DX.cover_tables(W)
    rng = np.random.default_rng(5)
    C = rng.uniform(0, 1, (4, T))
    Ct = C - C.mean(axis=1, keepdims=True)
    H = Ct @ Ct.T
    Q = pmd.r.astype(np.float64) * pmd.s.astype(np.float64)[None, :]
    Mt = (Q @ (pmd.v.astype(np.float64) @ Ct.T)).T
    a = DX.unit_columns(W)[t["perm"]]
    frozen = np.array([0, 0, 1, 0], dtype=np.int32)
    u_of_c = np.asarray(pmd.row_indices).reshape(-1)
    got = HR.hals_pixels(a.copy(), u_of_c[t["px"]], t["cov_ptr"], t["cov_k"], pmd.u.tocsr().astype(np.float64),
                         np.asarray(pmd.var_img, np.float64).reshape(-1)[t["px"]], Mt, H, frozen)
    S = (X - X.mean(axis=1, keepdims=True)) @ Ct.T
    want = a.copy()
    for q, p in enumerate(t["px"]):
        j0, j1 = t["cov_ptr"][q], t["cov_ptr"][q + 1]
        ks = t["cov_k"][j0:j1]
        want[j0:j1] = HR.gauss_seidel_pairs(a[j0:j1].copy(), S[p, ks], H[np.ix_(ks, ks)], frozen[ks] != 0)
    assert np.abs(got - want).max() <= 1e-11 * max(1.0, np.abs(want).max())
    assert np.array_equal(got[t["cov_k"] == 2], a[t["cov_k"] == 2]) and not np.array_equal(got, a)


# ---- argument checks -----------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_device_work(no_device):
    pmd = _small_pmd("F")
    T, d1, d2 = pmd.shape
    rois = _rois(d1, d2)
    for bad in (0, -1, 2.5, True, None, "3"):
        with pytest.raises(ValueError, match="outer_iters"):
            localmd_amd.demix(pmd, rois, outer_iters=bad)
        with pytest.raises(ValueError, match="sweeps"):
            pmd.demix(rois, sweeps=bad)
    with pytest.raises(ValueError, match="K = 0"):
        localmd_amd.demix(pmd, np.zeros((0, d1, d2)))
    with pytest.raises(ValueError, match="no pixels"):
        localmd_amd.demix(pmd, np.stack([rois[0], np.zeros((d1, d2), bool)]))
    with pytest.raises(ValueError, match="negative"):
        localmd_amd.demix(pmd, -rois.astype(np.float64))
    with pytest.raises(ValueError, match="covered by 65 ROIs"):
        localmd_amd.demix(pmd, np.ones((65, d1, d2), bool))
    with pytest.raises(ValueError, match="field of view"):
        localmd_amd.demix(pmd, np.ones((2, d1 + 1, d2), bool))
    with pytest.raises(TypeError):
        localmd_amd.demix(np.zeros((T, d1, d2)), rois)
    empty = PMDArray(scipy.sparse.csr_matrix((d1 * d2, 0)), np.zeros((0, 0), np.float32), np.zeros(0, np.float32),
                     np.zeros((0, T), np.float32), (T, d1, d2), "F", pmd.mean_img, pmd.var_img)
    with pytest.raises(ValueError, match="rank 0"):
        localmd_amd.demix(empty, rois)
    # 64 covers are allowed: the tables are built
    assert DX.cover_tables(roi_weights(np.ones((64, d1, d2), bool), (d1, d2), "F")[0])["cov_ptr"][1] == 64


def test_memory_plan_is_monotone_and_linear_in_k_t():
    base = dict(K=50, T=1000, n_pairs=5000, n_px=3000, nnz_g=400, nnz_b=9000, nnz_u=10 ** 6, n_rows=65536, n_cols=900,
                rank=120, factors_on_device=False)
    a = DX.demix_device_bytes(**base)
    assert DX.demix_device_bytes(**dict(base, T=5000)) - a == 8 * 50 * 4000
    assert DX.demix_device_bytes(**dict(base, T=9000)) - a == 8 * 50 * 8000
    for key in ("K", "T", "n_pairs", "n_px", "nnz_g", "nnz_b", "nnz_u", "n_rows", "n_cols", "rank"):
        assert DX.demix_device_bytes(**dict(base, **{key: 2 * base[key]})) > a, key
    assert DX.demix_device_bytes(**dict(base, factors_on_device=True)) < a
    # the part that does not grow with T is the same for every T, and K enters the growth as 8 T per ROI
    assert (DX.demix_device_bytes(**dict(base, K=51)) - a) - (DX.demix_device_bytes(**dict(base, K=51, T=2000))
                                                             - DX.demix_device_bytes(**dict(base, T=2000))) == -8 * 1000
    from localmd_amd._stream import check_fit
    with pytest.raises(ValueError, match="demix needs about"):
        check_fit("demix", a, a - 1)
