"""Host side of localmd_amd.grow (no GPU): the finish and its variance floor, windows, the pair and others tables against
the double loop of tests/grow_ref.py, the growing rule on hand-drawn correlation images, merge_rois, the argument checks
of the three functions, the device-memory plan, and the planted cells of test_gpu_superpixels.py through one and two
rounds of growing on the host."""
import importlib

import numpy as np
import pytest
import scipy.sparse

import localmd_amd
from localmd_amd import _lib
from localmd_amd._expand import expander_bytes
from localmd_amd._stream import BLOCK, batch_buffer_bytes
from localmd_amd.demix import Demixed
from tests import grow_ref as GR
from tests import hals_ref as HR
from tests.test_demix_host import _expand64, _small_pmd
from tests.test_traces_host import _disc

GX = importlib.import_module("localmd_amd.grow")


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a device context fails the test: the checks must come first."""
    def refuse(*a, **k):
        raise AssertionError("a device context was opened before the argument checks")
    monkeypatch.setattr(_lib.Context, "__init__", refuse)


# ---- the finish -----------------------------------------------------------------------------------------------------
def test_finish_against_corrcoef_and_least_squares():
    rng = np.random.default_rng(0)
    T, n = 400, 30
    y = rng.standard_normal((T, n)) * rng.uniform(0.1, 50, n) + rng.uniform(-100, 100, n)
    c = 0.3 * y + rng.standard_normal((T, n)) * rng.uniform(0.1, 5, n) + 7.0
    mom = np.stack([y.sum(axis=0), (y * y).sum(axis=0), (y * c).sum(axis=0)])
    rho, beta = GX.finish_moments(mom, T, c.sum(axis=0), (c * c).sum(axis=0))
    rho_ref, beta_ref = GR.finish(mom, T, c.sum(axis=0), (c * c).sum(axis=0))
    assert np.array_equal(rho, rho_ref) and np.array_equal(beta, beta_ref)
    for i in range(n):
        assert abs(rho[i] - np.corrcoef(y[:, i], c[:, i])[0, 1]) <= 1e-12
        slope = np.linalg.lstsq(np.stack([c[:, i], np.ones(T)], axis=1), y[:, i], rcond=None)[0][0]
        assert abs(beta[i] - slope) <= 1e-12 * max(1.0, abs(slope))


@pytest.mark.parametrize("T", (3, 1000, 4097))
def test_floor_on_signed_constant_columns(T):
    """Constant columns of either sign, summed by fp64 chains as the kernel does: the computed variance is rounding
    alone and lies at or below the floor, so rho = 0.  A column that differs from the constant in one frame by a relative
    0.1 has var / (T Syy) of about 1e-2 / T, so the floor's 3 (T + 2) 2^-53 is a relative 3 T (T + 2) 2^-51 of its
    variance, 6e-7 at T = 4097: it is live and |rho| = 1 to 1e-5.  The floor is that of superpixels.variance_floor."""
    SP = importlib.import_module("localmd_amd.superpixels")
    assert GX.variance_floor(T) == SP.variance_floor(T) == 3.0 * (T + 2) * 2.0 ** -53
    rng = np.random.default_rng(T)
    vals = np.concatenate([rng.uniform(-1e4, 1e4, 40), [-1.0 / 3.0, 0.1, -123456.789, 1e-30, -1e30]]).astype(np.float32)
    y = np.repeat(vals[None, :].astype(np.float64), T, axis=0)
    c = rng.standard_normal(T)
    mom = np.stack([np.cumsum(y, axis=0)[-1], np.cumsum(y * y, axis=0)[-1], np.cumsum(y * c[:, None], axis=0)[-1]])
    Sc, Scc = np.full(len(vals), c.sum()), np.full(len(vals), (c * c).sum())
    var = T * mom[1] - mom[0] ** 2
    assert np.all(np.abs(var) <= GX.variance_floor(T) * T * mom[1])
    rho, _ = GX.finish_moments(mom, T, Sc, Scc)
    assert np.array_equal(rho, np.zeros(len(vals)))
    # a constant trace against a live column: rho = 0 as well, beta whatever the division gives
    rho, _ = GX.finish_moments(np.stack([c.sum()[None], (c * c).sum()[None], (2.5 * c).sum()[None]]), T, [2.5 * T], [6.25 * T])
    assert rho[0] == 0.0
    y2 = y.copy()
    y2[T // 2] *= 1.1
    y2[T // 2, vals == 0] = 1.0
    c2 = np.zeros(T)
    c2[T // 2] = 1.0
    mom2 = np.stack([np.cumsum(y2, axis=0)[-1], np.cumsum(y2 * y2, axis=0)[-1], np.cumsum(y2 * c2[:, None], axis=0)[-1]])
    rho2, _ = GX.finish_moments(mom2, T, np.full(len(vals), 1.0), np.full(len(vals), 1.0))
    assert np.all(np.abs(np.abs(rho2) - 1.0) <= 1e-5)


def test_trace_sums_are_numpy_sums_of_the_float64_row():
    C = np.random.default_rng(1).standard_normal((4, 1000)).astype(np.float32)
    Sc, Scc = GX.trace_sums(C[:, ::2])                     # a strided view: the copy is what is summed
    for k in range(4):
        c = np.ascontiguousarray(C[k, ::2], dtype=np.float64)
        assert Sc[k] == np.sum(c) and Scc[k] == np.sum(c * c)


# ---- windows and tables ---------------------------------------------------------------------------------------------
def _corner_rois(d1, d2):
    m = np.zeros((6, d1, d2), np.float32)
    m[0, 0:2, 0:3] = 1
    m[1, 0:3, d2 - 2:] = 2
    m[2, d1 - 1:, 0:1] = 3
    m[3, d1 - 3:, d2 - 1:] = 4
    m[4, 5:8, 4:9] = 5
    return m                                                # ROI 5 is empty


def test_windows_at_the_corners_and_without_halo():
    d1, d2 = 12, 15
    A = _corner_rois(d1, d2).reshape(6, -1)
    for halo in (0, 1, 4, 20):
        want = GR.windows(A, d1, d2, halo)
        got = GX.windows(GX.supports(scipy.sparse.csr_matrix(A)), d1, d2, halo)
        for k in range(6):
            assert tuple(got[k]) == want.get(k, (0, 0, 0, 0)), (halo, k)
    assert tuple(GX.windows(GX.supports(scipy.sparse.csr_matrix(A)), d1, d2, 0)[4]) == (5, 8, 4, 9)
    assert tuple(GX.windows(GX.supports(scipy.sparse.csr_matrix(A)), d1, d2, 20)[0]) == (0, d1, 0, d2)


def test_supports_ignore_explicit_zeros():
    A = scipy.sparse.csr_matrix((np.array([1.0, 0.0, 2.0], np.float32), np.array([3, 4, 7]), np.array([0, 3])), shape=(1, 9))
    S = GX.supports(A)
    assert list(S.indices) == [3, 7]
    # the footprints themselves are left alone: demix returns them with the zeros HALS has set, stored explicitly
    assert A.nnz == 3 and list(A.indices) == [3, 4, 7] and list(A.indptr) == [0, 3] and list(A.data) == [1.0, 0.0, 2.0]
    t = GX.pair_tables(A, np.array([[0, 1, 0, 9]]), np.array([True]), 9)
    assert list(t["pair_px"]) == list(range(9)) and len(t["oth_k"]) == 0 and A.nnz == 3


@pytest.mark.parametrize("n_cover", (1, 2, 64))
def test_pair_and_other_tables_against_the_double_loop(n_cover):
    """n_cover ROIs stacked on the same pixels (0, 1 and 63 others inside, and n_cover = 64 others on the halo of a
    65th ROI next to them), plus a fixed ROI that gets no pairs and still shows up among the others."""
    d1, d2 = 9, 11
    rng = np.random.default_rng(n_cover)
    K = n_cover + 2
    A = np.zeros((K, d1, d2), np.float32)
    A[:n_cover, 2:5, 3:6] = rng.uniform(0.5, 2, (n_cover, 3, 3))
    A[n_cover, 2:5, 6:8] = 1.5                               # its halo reaches the stack: n_cover others there
    A[n_cover + 1, 1:3, 2:5] = 0.25                          # fixed
    A = A.reshape(K, -1)
    movable = np.ones(K, bool)
    movable[K - 1] = False
    if n_cover == 64:
        with pytest.raises(ValueError, match="at most 64"):
            GX.pair_tables(scipy.sparse.csr_matrix(A), np.zeros((K, 4), np.int64), movable, d2)
        A[K - 1] = 0                                         # without the fixed ROI on top of the stack: 64 cover it
    win = GX.windows(GX.supports(scipy.sparse.csr_matrix(A)), d1, d2, 2)
    t = GX.pair_tables(scipy.sparse.csr_matrix(A), win, movable, d2)
    px, pk, others = GR.tables(A, GR.windows(A, d1, d2, 2), movable, d2)
    assert t["pair_px"].dtype == np.int32 and t["pair_k"].dtype == np.int32 and t["oth_ptr"].dtype == np.int64
    assert t["oth_k"].dtype == np.int32 and t["oth_a"].dtype == np.float32
    assert list(t["pair_px"]) == px and list(t["pair_k"]) == pk
    assert t["oth_ptr"][0] == 0 and t["oth_ptr"][-1] == len(t["oth_k"]) == len(t["oth_a"])
    counts = set()
    for i in range(len(px)):
        q0, q1 = t["oth_ptr"][i], t["oth_ptr"][i + 1]
        assert [(int(l), a) for l, a in zip(t["oth_k"][q0:q1], t["oth_a"][q0:q1])] == [(l, a) for l, a in others[i]], i
        counts.add(int(q1 - q0))
    assert {0, n_cover - 1, n_cover} <= counts
    assert np.array_equal(np.diff(t["roi_ptr"]), np.bincount(np.asarray(pk), minlength=K))
    assert t["roi_ptr"][K] - t["roi_ptr"][K - 1] == 0


# ---- the growing rule -----------------------------------------------------------------------------------------------
def _rho_image():
    """9 x 9: the seed in the middle, one of its pixels with a NaN rho; a candidate arm that touches it only diagonally;
    an island that does not touch it."""
    rho = np.full((9, 9), 0.1)
    seed = np.zeros((9, 9), bool)
    seed[3:5, 3:5] = True
    rho[3:5, 3:5] = 0.9
    rho[5, 5], rho[6, 6] = 0.85, 0.75      # (5, 5) touches (4, 4) diagonally and nothing else of the seed
    rho[0:2, 7:9] = 0.95                   # an island
    rho[3, 3] = np.nan                     # a non-finite rho is no candidate
    return rho, seed


def test_growing_rule_on_hand_drawn_images():
    rho, seed = _rho_image()
    for fn in (GX.grow_support, GR.grow_rule):
        new, th, status = fn(rho, seed, 0.6)
        want = seed.copy()
        want[3, 3] = False
        want[5, 5] = want[6, 6] = True                       # the arm hangs on a diagonal; the island stays out
        assert status == "grown" and th == 0.6 and np.array_equal(new, want)
        new, th, status = fn(rho, seed, 0.6, shrink=False)
        want[3, 3] = True
        assert status == "grown" and np.array_equal(new, want)
        # lost: no candidate on the seed, with shrink on and off
        new, th, status = fn(np.where(seed, 0.5, rho), seed, 0.6)
        assert new is None and status == "lost" and th == 0.6
        new, th, status = fn(np.where(seed, 0.5, rho), seed, 0.6, shrink=False)
        assert new is None and status == "lost"
        # max_size: 5 pixels at 0.6 and at 0.7, 4 at 0.6 + 0.1 + 0.1 (0.75 drops out), 3 one step later (0.85 does)
        new, th, status = fn(rho, seed, 0.6, max_size=4)
        assert status == "grown" and th == 0.6 + 0.1 + 0.1 and new.sum() == 4 and not new[6, 6] and new[5, 5]
        new, th, status = fn(rho, seed, 0.6, max_size=3)
        assert status == "grown" and th == 0.6 + 0.1 + 0.1 + 0.1 and new.sum() == 3 and not new[5, 5]
        # 0.6 + 0.1 + 0.1 + 0.1 + 0.1 = 0.9999999999999999 < 1 is one more step, and nothing is above it
        new, th, status = fn(rho, seed, 0.6, max_size=2)
        assert new is None and status == "lost" and th == 0.6 + 0.1 + 0.1 + 0.1 + 0.1 < 1
    flat = np.full((9, 9), 0.99)
    for fn in (GX.grow_support, GR.grow_rule):
        new, th, status = fn(flat, seed, 0.55, max_size=10)
        assert new is None and status == "oversize"
        assert th == 0.55 + 0.1 + 0.1 + 0.1 + 0.1 and not th + 0.1 < 1                # 0.95: the next step would reach 1
        new, th, status = fn(flat, seed, -1.0, max_size=81)
        assert status == "grown" and th == -1.0 and new.all()


def _fake_demixed(A, C, empty=None, labels=None):
    A = scipy.sparse.csr_matrix(np.asarray(A, np.float32))
    K = A.shape[0]
    return Demixed(np.asarray(C, np.float32), A, None, np.arange(K) + 10 if labels is None else labels, None,
                   np.zeros(K, bool) if empty is None else empty)


def test_grow_all_statuses_fixed_max_window_and_empty():
    d1, d2 = 12, 15
    A = _corner_rois(d1, d2).reshape(6, -1)
    S = GX.supports(scipy.sparse.csr_matrix(A))
    win = GX.windows(S, d1, d2, 2)
    status = GX.roi_status(S, win, GX.fixed_mask(6, [1]), 30)
    # windows: 4 x 5 = 20, (fixed), 3 x 3 = 9, 5 x 3 = 15, 7 x 9 = 63 > 30, empty
    assert list(status) == ["grown", "fixed", "grown", "grown", "fixed", "empty"]
    assert list(GX.roi_status(S, win, GX.fixed_mask(6, np.array([0, 0, 1, 0, 0, 1], bool)), 63)) == \
        ["grown", "grown", "fixed", "grown", "grown", "empty"]
    t = GX.pair_tables(scipy.sparse.csr_matrix(A), win, status == "grown", d2)
    n = len(t["pair_px"])
    assert n == 20 + 9 + 15
    rho = np.zeros(n)
    beta = np.full(n, 0.5)
    rho[:20] = 0.9                                           # ROI 0: its whole window; ROI 2: nothing; ROI 3: its seed
    rho[20 + 9:] = np.where(A[3, t["pair_px"][29:]] > 0, 0.7, 0.2)
    rows, th, added, removed, status2 = GX.grow_all(scipy.sparse.csr_matrix(A), t, win, status, rho, beta, d2, 0.6, True,
                                                    None)
    assert list(status2) == ["grown", "fixed", "lost", "grown", "fixed", "empty"]
    assert list(added) == [14, 0, 0, 0, 0, 0] and list(removed) == [0] * 6
    assert rows[0][0].size == 20 and np.all(rows[0][1] == np.float32(0.5))
    for k in (1, 2, 4):                                      # kept as they are, bit for bit
        assert np.array_equal(rows[k][0], np.nonzero(A[k])[0]) and np.array_equal(rows[k][1], A[k][A[k] > 0])
    assert rows[5][0].size == 0
    assert np.array_equal(rows[3][0], np.nonzero(A[3])[0]) and np.all(rows[3][1] == np.float32(0.5))


def test_shrink_false_keeps_old_values_where_beta_is_not_positive():
    d1, d2 = 6, 6
    A = np.zeros((1, d1, d2), np.float32)
    A[0, 2:4, 2:4] = [[1, 2], [3, 4]]
    A = A.reshape(1, -1)
    S = GX.supports(scipy.sparse.csr_matrix(A))
    win = GX.windows(S, d1, d2, 1)
    status = GX.roi_status(S, win, GX.fixed_mask(1, None), 100)
    t = GX.pair_tables(scipy.sparse.csr_matrix(A), win, status == "grown", d2)
    px = t["pair_px"]
    rho = np.where(np.isin(px, [14, 15, 16]), 0.9, -0.5)     # (2, 2), (2, 3) and a new pixel (2, 4)
    beta = np.where(rho > 0, 0.75, -0.25)
    beta[px == 21] = np.nan                                  # (3, 3): not > 0 either
    rows, _, added, removed, _ = GX.grow_all(scipy.sparse.csr_matrix(A), t, win, status, rho, beta, d2, 0.6, False, None)
    assert list(rows[0][0]) == [14, 15, 16, 20, 21] and list(rows[0][1]) == [0.75, 0.75, 0.75, 3.0, 4.0]
    assert added[0] == 1 and removed[0] == 0
    rows, _, added, removed, _ = GX.grow_all(scipy.sparse.csr_matrix(A), t, win, status, rho, beta, d2, 0.6, True, None)
    assert list(rows[0][0]) == [14, 15, 16] and added[0] == 1 and removed[0] == 2


# ---- merge_rois -----------------------------------------------------------------------------------------------------
def _merge_case():
    """Six ROIs on 40 pixels.  0 and 1 overlap by 4 of 5 and correlate; 2 overlaps 1 by 4 of 5 and correlates with 1 (a
    chain 0 - 1 - 2 although 0 and 2 share nothing); 3 overlaps 4 by 4 of 5 without correlating; 5 correlates with 4 and
    overlaps it by 1 of 5."""
    rng = np.random.default_rng(5)
    A = np.zeros((6, 40), np.float32)
    A[0, 0:5], A[1, 1:6], A[2, 5:10] = rng.uniform(0.5, 2, (3, 5))
    A[2, 1:5] = 0
    A[2, 2:6] = rng.uniform(0.5, 2, 4)
    A[2, 6] = 1.0
    A[3, 20:25], A[4, 21:26], A[5, 25:30] = rng.uniform(0.5, 2, (3, 5))
    base = rng.standard_normal((3, 300))
    C = np.stack([base[0], base[0] + 0.1 * rng.standard_normal(300), base[0] + 0.1 * rng.standard_normal(300),
                  base[1], base[2], base[2] + 0.05 * rng.standard_normal(300)]).astype(np.float32)
    return A, C


def test_merge_rois_conditions_chains_singletons_and_fixed():
    A, C = _merge_case()
    assert not (A[0] > 0)[np.nonzero(A[2])[0]].sum() / 5 > 0.6          # 0 and 2 alone would not merge
    labels = np.array([7, 3, 9, 4, 5, 6])
    m = localmd_amd.merge_rois(scipy.sparse.csr_matrix(A), C, labels=labels)
    rows, groups = GR.merge(A, C)
    assert [list(g) for g in m.groups] == groups == [[0, 1, 2], [3], [4], [5]]
    assert list(m.labels) == [7, 4, 5, 6]
    got = m.rois.toarray()
    assert m.rois.dtype == np.float32 and m.rois.has_sorted_indices
    # the merged row: a float64 sum of three products rounded to float32 once; the two statements form the norms in a
    # different order of summation, a relative 300 * 2^-53 apart, far inside one float32 rounding of the row
    np.testing.assert_allclose(got[0], rows[0], rtol=2.0 ** -23, atol=0)
    assert np.array_equal(got[0] > 0, (A[:3] > 0).any(axis=0))
    for out_row, k in ((1, 3), (2, 4), (3, 5)):               # singletons: bit for bit
        assert got[out_row].tobytes() == A[k].tobytes()
    # thresholds are strict and each condition alone does not merge
    assert [list(g) for g in localmd_amd.merge_rois(A, C, overlap_th=0.8).groups] == [[k] for k in range(6)]
    assert [list(g) for g in localmd_amd.merge_rois(A, C, corr_th=0.999).groups] == [[k] for k in range(6)]
    assert [list(g) for g in localmd_amd.merge_rois(A, C, overlap_th=0.1, corr_th=0.9).groups] == [[0, 1, 2], [3], [4, 5]]
    # fixed rows never merge: without 1 the chain falls apart
    assert [list(g) for g in localmd_amd.merge_rois(A, C, fixed=[1]).groups] == [[k] for k in range(6)]
    assert [list(g) for g in localmd_amd.merge_rois(A, C, fixed=np.array([1, 0, 0, 0, 0, 0], bool)).groups] == \
        [[0], [1, 2], [3], [4], [5]]
    assert [list(g) for g in GR.merge(A, C, fixed=[True, False, False, False, False, False])[1]] == [[0], [1, 2], [3], [4], [5]]
    # a constant trace correlates with nothing
    C0 = C.copy()
    C0[0] = 3.0
    assert [list(g) for g in localmd_amd.merge_rois(A, C0).groups][:2] == [[0], [1, 2]]


# ---- argument checks ------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_device_work(no_device):
    pmd = _small_pmd("C")
    T, d1, d2 = pmd.shape
    D = d1 * d2
    A = np.zeros((2, D), np.float32)
    A[0, 11:14], A[1, 50:53] = 1, 2
    dm = _fake_demixed(A, np.ones((2, T)))
    bad = [dict(kind="residual"), dict(corr_th=1.0), dict(corr_th=np.nan), dict(corr_th="x"), dict(halo=-1), dict(halo=1.5),
           dict(shrink=1), dict(max_size=0), dict(max_size=2.0), dict(max_window=0), dict(fixed=[2]), dict(fixed=[-1]),
           dict(fixed=np.zeros(3, bool)), dict(fixed=[0.5]), dict(kind="raw")]
    for kw in bad:
        with pytest.raises(ValueError):
            localmd_amd.grow_rois(pmd, dm, **kw)
    with pytest.raises(TypeError):
        localmd_amd.grow_rois("pmd", dm)
    with pytest.raises(TypeError):
        localmd_amd.grow_rois(pmd, A)
    with pytest.raises(ValueError, match="traces"):
        localmd_amd.grow_rois(pmd, _fake_demixed(A, np.ones((2, T + 1))))
    with pytest.raises(ValueError, match="footprints"):
        localmd_amd.grow_rois(pmd, _fake_demixed(A[:, :-1], np.ones((2, T))))
    with pytest.raises(ValueError, match="negative"):
        localmd_amd.grow_rois(pmd, _fake_demixed(-A, np.ones((2, T))))
    with pytest.raises(ValueError, match="shape"):
        localmd_amd.grow_rois(pmd, dm, np.zeros((T, d1, d2 + 1), np.float32), kind="raw")
    # every ROI fixed: nothing to do on the device, the ROIs come back as they are
    g = pmd.grow_rois(dm, fixed=[0, 1])
    assert list(g.status) == ["fixed", "fixed"] and g.rois.toarray().tobytes() == A.tobytes() and g.correlation.nnz == 0
    assert list(g.labels) == [10, 11] and list(g.source) == [0, 1]

    for kw in (dict(corr_th=1.0), dict(overlap_th=1.0), dict(overlap_th=-0.1), dict(fixed=[5]), dict(labels=np.arange(3))):
        with pytest.raises(ValueError):
            localmd_amd.merge_rois(A, np.ones((2, T)), **kw)
    with pytest.raises(ValueError):
        localmd_amd.merge_rois(A, np.ones((3, T)))
    with pytest.raises(ValueError):
        localmd_amd.merge_rois(-A, np.ones((2, T)))
    with pytest.raises(ValueError):
        localmd_amd.merge_rois(A.reshape(2, d1, d2), np.ones((2, T)))

    rois = A.reshape(2, d1, d2)
    for kw in (dict(rounds=-1), dict(rounds=1.5), dict(merge_kw=dict(fixed=[0]))):
        with pytest.raises(ValueError):
            localmd_amd.refine_demix(pmd, rois, **kw)
    with pytest.raises(TypeError):
        localmd_amd.refine_demix("pmd", rois)
    with pytest.raises(ValueError):
        pmd.refine_demix(-rois)                              # demix's own check, still before the device


def test_grow_device_bytes_term_by_term():
    base = dict(D=4096, nb=2048, esize=2, n_cols=300, rank=40, n_entries=500, n_a=9000, n_patches=64, host_source=True,
                n_batches=3, factors_on_device=False, kind="denoised", K=50, n_pairs=10000, n_others=700)
    ex = dict(D=4096, n_cols=300, rank=40, n_entries=500, n_a=9000, n_patches=64, factors_on_device=False, block_panels=1)
    slack = 1 << 20
    assert GX.grow_device_bytes(**base) == 32 * 10000 + 8 * 10001 + 8 * 700 + 4 * 50 * BLOCK + expander_bytes(**ex) + slack
    assert GX.grow_device_bytes(**dict(base, n_pairs=10001)) - GX.grow_device_bytes(**base) == 24 + 8 + 8
    assert GX.grow_device_bytes(**dict(base, n_others=701)) - GX.grow_device_bytes(**base) == 8
    assert GX.grow_device_bytes(**dict(base, K=51)) - GX.grow_device_bytes(**base) == 4 * BLOCK
    raw = GX.grow_device_bytes(**dict(base, kind="raw"))
    assert raw == 32 * 10000 + 8 * 10001 + 8 * 700 + 4 * 50 * BLOCK + batch_buffer_bytes(2048, 4096, 2, True, 3) + slack
    assert GX.grow_device_bytes(**dict(base, kind="raw", host_source=False)) == raw - 2048 * 4096 * 2
    on = GX.grow_device_bytes(**dict(base, factors_on_device=True))
    assert GX.grow_device_bytes(**base) - on == 4 * 300 * 40


def test_in_pixel_order():
    d1, d2 = 3, 4
    R = scipy.sparse.csr_matrix(np.arange(24, dtype=np.float32).reshape(2, 12))
    assert GX.in_pixel_order(R, (d1, d2), "C") is R
    F = GX.in_pixel_order(R, (d1, d2), "F").toarray()
    for i in range(d1):
        for j in range(d2):
            assert F[1, j * d1 + i] == R[1, i * d2 + j]


# ---- the planted cells ----------------------------------------------------------------------------------------------
def _seeds(d1, d2, cells):
    return np.stack([_disc(d1, d2, ci, cj, r - 1.3) for ci, cj, r in cells])


def planted_round(X64, A0, S, C_true, masks, d1, d2, corr_th=0.8, halo=4):
    """One demix_ref on the supports S ((K, D) bool) with weights A0, then one grow_ref.  Returns (demix, grown, 1 - corr
    of every trace with the planted one)."""
    dm = HR.demix_ref(X64, A0.T.astype(np.float64), S.T)
    A = dm["footprints"].T.astype(np.float32)
    C = dm["traces"].astype(np.float32)
    X = X64.T.reshape(-1, d1, d2).astype(np.float32)
    g = GR.grow_ref(X, A, C, d1, d2, corr_th=corr_th, halo=halo)
    miss = [1.0 - float(np.corrcoef(dm["traces"][k], C_true[k])[0, 1]) for k in range(len(C_true))]
    return dm, g, miss


def _rows_dense(rows, K, D):
    A = np.zeros((K, D), np.float32)
    for k, (idx, val) in rows.items():
        A[k, idx] = val
    return A


def test_planted_cells_grow_back_on_the_host():
    """Measured with tests/grow_ref.py and tests/hals_ref.demix_ref on the host expansion of the planted movie of
    test_gpu_superpixels.py (seed 3; 24 x 28 x 600, cells of 29, 25, 21, 37, 37 pixels, cells 3 and 4 sharing 14), from
    disc seeds of radius r - 1.3 (9, 9, 5, 13, 13 pixels), corr_th = 0.8, halo = 4; the figures are printed by this test
    (pytest -s) and were, with the committed reference:

    round 1: missing pixels per cell 0, 0, 0, 1, 2, none extra; smallest |rho - corr_th| = 1.8e-2;
             1 - corr with the planted traces before / after re-demixing: cell 3 2.34e-2 -> 7.9e-4 (29.8x), cell 4
             4.55e-2 -> 5.8e-4 (78.5x);
    round 2: missing 0, 0, 0, 1, 1, none extra; smallest |rho - corr_th| = 1.1e-2.

    Asserted: the three isolated cells exactly, no pixel outside a cell in any support (pixels outside every cell are
    constant: rho = 0 against about 1 inside), and 1 - corr of cells 3 and 4 down by at least 4x after one round."""
    from tests.test_gpu_superpixels import CELLS, _planted_cells

    pmd, masks, traces = _planted_cells()
    T, d1, d2 = pmd.shape
    D = d1 * d2
    K = len(CELLS)
    X64 = _expand64(pmd)
    M = masks.reshape(K, D)
    S = _seeds(d1, d2, CELLS).reshape(K, D)
    assert list(S.sum(axis=1)) == [9, 9, 5, 13, 13] and not (S & ~M).any()
    dm0, g1, miss0 = planted_round(X64, S.astype(np.float64), S, traces, masks, d1, d2)
    A1 = _rows_dense(g1["rows"], K, D)
    S1 = A1 > 0
    missing1 = [int((M[k] & ~S1[k]).sum()) for k in range(K)]
    print("round 1: status", g1["status"], "missing", missing1, "extra", int((S1 & ~M).sum()), "margin", g1["margin"])
    assert g1["status"] == ["grown"] * K
    assert g1["margin"] >= 1e-6                               # a property of the input: decisions far from fp32 effects
    for k in (0, 1, 2):
        assert np.array_equal(S1[k], M[k]), k
    assert not (S1 & ~M).any()
    assert max(missing1[3:]) <= 3
    dm1, g2, miss1 = planted_round(X64, A1, S1, traces, masks, d1, d2)
    print("1 - corr before", miss0, "after one round", miss1, "gain", [a / b if b else np.inf for a, b in zip(miss0, miss1)])
    for k in (3, 4):
        assert miss1[k] * 4.0 <= miss0[k], (k, miss0[k], miss1[k])
    S2 = _rows_dense(g2["rows"], K, D) > 0
    missing2 = [int((M[k] & ~S2[k]).sum()) for k in range(K)]
    print("round 2: status", g2["status"], "missing", missing2, "extra", int((S2 & ~M).sum()), "margin", g2["margin"])
    for k in (0, 1, 2):
        assert np.array_equal(S2[k], M[k]), k
    assert not (S2 & ~M).any()
