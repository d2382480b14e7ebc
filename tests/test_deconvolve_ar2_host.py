"""Host side of localmd_amd.deconvolve(p=2) (no device): the NumPy restatement of the OASIS AR(2) solver
(tests/oasis2_ref.py) against the AR(1) restatement at g2 = 0, against direct least-squares fits of its pools, against
scipy's NNLS and against itself in fp32; the tables, the ceiling of the search, the estimate of (g1, g2), the argument
checks, the launch and memory plans, and the planted-event and onset properties through the package's own search."""
import functools
import importlib

import numpy as np
import pytest

import localmd_amd
from tests import oasis2_ref as R2
from tests import oasis_ref as R1

DX = importlib.import_module("localmd_amd.deconvolve")     # the module: the package exports the function under the same name

SIGMA = 0.3
PAIRS = ((0.9, 0.3), (0.95, 0.5), (0.97, 0.8))             # (d, r): decay and rise roots
# Relative objective excess of the greedy float64 form over scipy's NNLS, (obj - obj_nnls) / obj_nnls, the largest over
# T in {300, 800} x lam in {0, 0.3, 1} on planted2(seed=T), as planted and with a first sample of -3 (whose largest are
# 2.52e-3, 7.49e-3 and 3.23e-2), per pair, as measured; the bound is twice that (the factor only absorbs BLAS and NNLS
# differences between machines: the inputs and the float64 form are deterministic).
GREEDY_EXCESS = {(0.9, 0.3): 3.60e-3, (0.95, 0.5): 1.052e-2, (0.97, 0.8): 4.49e-2}
# fp32 emulation against the float64 form on the inputs of test_emulation_tracks_float64, as a fraction of max |y|: the
# largest value measured over its 36 cases, all with equal pool counts, is 4.71e-7 (T = 4097, d = r = 0.9, lam = 2); the
# bound is four times that, the rule of tests/test_deconvolve_host.py.
EMULATION_ERR2 = 4.71e-7
# |d^ - d| and |r^ - r| of estimate_ar2 at T = 10^4, sigma = 0.3, seeds 11 .. 14 of planted2, the largest per pair as
# measured; the bounds are twice that.
ESTIMATE_ERR = {(0.9, 0.3): (0.0132, 0.145), (0.95, 0.5): (0.00749, 0.183), (0.97, 0.8): (0.0101, 0.326)}
PLANTED = ((1, 0.015), (2, 0.02), (3, 0.01))               # (seed, event rate): d = 0.95, r = 0.5, T = 3000


def pair(d, r):
    g = DX.ar2_from_roots(d, r)
    return float(g[0]), float(g[1])


def roots(g):
    g = np.atleast_2d(g)
    root = np.sqrt(np.maximum(g[:, 0] ** 2 + 4 * g[:, 1], 0.0))
    return (g[:, 0] + root) / 2, (g[:, 0] - root) / 2


# ---- the solver's arithmetic ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,g", [(1, 0.95), (2, 0.5), (3, 0.9), (4, 0.0)])
def test_without_g2_it_is_the_ar1_solver(seed, g):
    """g2 = 0: calcium and spikes of the float64 form are those of oasis_ref.oasis_ar1 in float64 whenever s_min = 0, and
    with s_min > 0 whenever the first pool of the AR(1) form is positive (a first pool of negative value with s_min > 0:
    test_without_g2_a_negative_start_and_a_threshold).  The pool count is the same wherever that first pool is positive;
    where it is not, the AR(1) form keeps its leading pools of negative value apart and fills them with 0, while this
    form clips the value of its bottom pool in the forward pass (the pool above has to see the value c really takes), so
    those pools merge into one: fewer pools, the same c.  The trace as planted, with a large and with a strongly
    negative first sample."""
    y0, _, _ = R1.planted(seed, T=500, g=g if g else 0.5)
    kinds = set()
    for first in (None, 4.0, -3.0):
        y = y0.copy()
        if first is not None:
            y[0] = first
        for lam in (0.0, 0.3, 1.0):
            for s_min in (0.0, 0.2):
                c1, s1, rss1, n1 = R1.oasis_ar1(y, g, lam, s_min, dtype=np.float64)
                c2, s2, rss2, n2 = R2.oasis_ar2(y, g, 0.0, lam, s_min, dtype=np.float64)
                if s_min == 0 or c1[0] > 0:
                    assert np.abs(c1 - c2).max() <= 1e-12 * np.abs(y).max()
                    assert np.abs(s1 - s2).max() <= 1e-12 * np.abs(y).max()
                    assert rss2 == pytest.approx(rss1, rel=1e-12)
                if c1[0] > 0:
                    assert n2 == n1
                    kinds.add("positive start")
                elif s_min == 0:
                    assert n2 <= n1
                    kinds.add("clipped start")
    assert kinds == {"positive start", "clipped start"}


def negative_start(i, T=80, noise=0.5):
    """Noise, three events of height 2 and a first sample of -3: the bottom pool takes in frames by merges, and its fit
    is below 0 for a while."""
    rng = np.random.default_rng(1000 + i)
    y = noise * rng.standard_normal(T)
    y[rng.integers(5, T - 5, 3)] += 2.0
    y[0] = -3.0
    return y.astype(np.float32)


def test_without_g2_a_negative_start_and_a_threshold():
    """g2 = 0 on traces that start at -3.  With s_min = 0 calcium is that of the AR(1) form.  With s_min = 0.2 it is not
    (measured: up to 0.35 apart over these 100 traces and two decays): the AR(1) form compares the pool after its
    negative first pool with g^l times that negative value, which it later fills with 0, so its first spike can lie
    below s_min; here the bottom pool's value is clipped before the comparison and every spike is at least s_min."""
    apart, below = 0.0, 0
    for i in range(100):
        y = negative_start(i)
        for g in (0.9, 0.5):
            c1 = R1.oasis_ar1(y, g, 0.2, 0.0, dtype=np.float64)[0]
            c2 = R2.oasis_ar2(y, g, 0.0, 0.2, 0.0, dtype=np.float64)[0]
            assert np.abs(c1 - c2).max() <= 1e-12 * np.abs(y).max()
            c1, s1, _, _ = R1.oasis_ar1(y, g, 0.2, 0.2, dtype=np.float64)
            c2, s2, _, _ = R2.oasis_ar2(y, g, 0.0, 0.2, 0.2, dtype=np.float64)
            assert np.all(s2[s2 > 0] >= 0.2 - 1e-12) and np.all(c2 >= 0) and c2[0] == 0
            apart = max(apart, np.abs(c1 - c2).max())
            below += bool(np.any((s1 > 0) & (s1 < 0.2 - 1e-12)))
    print("s_min = 0.2: calcium of the two forms apart by", apart, "; AR(1) runs with a spike below s_min:", below)
    assert below > 0          # the inputs do reach the case


@functools.lru_cache(maxsize=None)
def greedy_case(d, r, T, lam, first=None):
    """planted2(seed=T), with ``first`` as its first sample when given (-3: frames merge into a bottom pool whose fit is
    below 0)."""
    y, _, _ = R2.planted2(T, T=T, d=d, r=r, sigma=SIGMA, rate=0.015)
    if first is not None:
        y = y.copy()
        y[0] = first
    g1, g2 = d + r, -d * r
    return (y, g1, g2) + R2.oasis_ar2(y, g1, g2, lam, dtype=np.float64, pools=True)


def pool_fit_error(y, g1, g2, lam, c, pools):
    """The largest |v - fit| over the pools: fit is the least-squares fit of c[t0 + j] = h_j v + g2 h_{j-1} w' to the
    penalised data with w' held fixed, clipped at 0 for the bottom pool."""
    T = len(y)
    h = R2.tables(g1, g2, T, np.float64)[0]
    pen = np.full(T, lam * (1 - g1 - g2))
    pen[-2], pen[-1] = lam * (1 - g1), lam
    yp = y.astype(np.float64) - pen
    worst = 0.0
    for k, (t0, l, v, gw) in enumerate(pools):
        a, fixed = h[1:l + 1], h[:l] * gw
        fit = float(a @ (yp[t0:t0 + l] - fixed)) / float(a @ a)
        if k == 0:
            fit = max(fit, 0.0)
        worst = max(worst, abs(fit - v))
        assert np.abs(c[t0:t0 + l] - (a * v + fixed)).max() <= 1e-12
    return worst


@pytest.mark.parametrize("first", [None, -3.0])
@pytest.mark.parametrize("T", [300, 800])
@pytest.mark.parametrize("d,r", PAIRS + ((0.95, 0.0), (0.9, 0.9)))
@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
def test_float64_form_is_feasible_and_fits_every_pool(T, d, r, lam, first):
    y, g1, g2, c, s, rss, n_pools, pools = greedy_case(d, r, T, lam, first)
    obj, s_min = R2.objective(y, c, g1, g2, lam)
    assert s_min >= -1e-12 and np.all(c >= 0) and np.all(s >= 0) and s[0] == 0
    res = y.astype(np.float64) - c
    assert rss == pytest.approx(float(res @ res), rel=1e-12)
    assert len(pools) == n_pools and sum(p[1] for p in pools) == T
    if first is not None:
        assert pools[0][1] > 1 or pools[0][2] == 0       # frames merged into the bottom pool, or it stayed at 0
    worst = pool_fit_error(y, g1, g2, lam, c, pools)
    print("T", T, "roots", d, r, "lam", lam, "first", first, "pool value - least-squares fit", worst)
    assert worst <= 1e-12


def test_a_negative_first_sample_counts_in_every_refit_of_the_bottom_pool():
    """200 short traces that start at -3 (noise 0.5, roots (0.95, 0.5), lam = 0.2): the bottom pool grows by merges while
    its sum N is negative and later turns positive.  Its value is the clipped least-squares fit of all its frames, the
    first included: the clip applies to v and w, never to N."""
    g1, g2 = 0.95 + 0.5, -0.95 * 0.5
    grown = forgetful = 0
    for i in range(200):
        y = negative_start(i)
        c, s, rss, n_pools, pools = R2.oasis_ar2(y, g1, g2, 0.2, dtype=np.float64, pools=True)
        assert pool_fit_error(y, g1, g2, 0.2, c, pools) <= 1e-12
        assert R2.objective(y, c, g1, g2, 0.2)[1] >= -1e-12 and np.all(c >= 0)
        grown += pools[0][1] > 1
        # a solver that forgot the first sample (N clipped with v) is this solver on the trace with y'[0] = 0: on some of
        # these traces its bottom pool is not the fit of the trace it was given, so the inputs can tell the two apart
        z = y.copy()
        z[0] = np.float32(0.2 * (1 - g1 - g2))
        cz, _, _, _, pz = R2.oasis_ar2(z, g1, g2, 0.2, dtype=np.float64, pools=True)
        h = R2.tables(g1, g2, len(y), np.float64)[0]
        l0 = pz[0][1]
        fit = max(0.0, float(h[1:l0 + 1] @ (y[:l0].astype(np.float64) - 0.2 * (1 - g1 - g2))) / float(h[1:l0 + 1] @ h[1:l0 + 1]))
        forgetful += abs(fit - pz[0][2]) > 1e-6
    print("bottom pools that took in frames:", grown, "; traces on which forgetting the first sample shows:", forgetful)
    assert grown >= 100 and forgetful >= 3


@pytest.mark.parametrize("d,r", PAIRS)
def test_greedy_gap_to_nnls(d, r):
    worst = 0.0
    for T in (300, 800):
        for first in (None, -3.0):
            for lam in (0.0, 0.3, 1.0):
                y, g1, g2, c = greedy_case(d, r, T, lam, first)[:4]
                cn, sn = R2.nnls_ref2(y, g1, g2, lam)
                obj, obj_n = R2.objective(y, c, g1, g2, lam)[0], R2.objective(y, cn, g1, g2, lam)[0]
                excess = (obj - obj_n) / obj_n
                print("roots", d, r, "T", T, "first", first, "lam", lam, "objective excess over nnls", excess)
                assert excess >= -1e-9
                worst = max(worst, excess)
    assert worst <= 2 * GREEDY_EXCESS[(d, r)]


@pytest.mark.parametrize("first", [None, -3.0])
@pytest.mark.parametrize("T", [300, 800])
def test_without_a_rise_the_greedy_solver_is_exact(T, first):
    """r = 0 is the AR(1) problem, where pooling is exact: the objective is that of NNLS on the Toeplitz problem, to the
    1e-9 that the gap test allows NNLS itself."""
    for lam in (0.0, 0.3, 1.0):
        y, g1, g2, c = greedy_case(0.95, 0.0, T, lam, first)[:4]
        cn, sn = R2.nnls_ref2(y, g1, g2, lam)
        obj, obj_n = R2.objective(y, c, g1, g2, lam)[0], R2.objective(y, cn, g1, g2, lam)[0]
        assert abs(obj - obj_n) <= 1e-9 * obj_n
        assert np.abs(c - cn).max() <= 1e-6 * np.abs(y).max()


def test_rss_is_monotone_in_the_penalty():
    y, _, _ = R2.planted2(5, T=400, d=0.95, r=0.5, sigma=SIGMA)
    g1, g2 = pair(0.95, 0.5)
    hi = float(DX.lambda_ceiling(y[None], np.float32([[g1, g2]]), np.float32([0]))[0])
    rss = [R2.oasis_ar2(y, g1, g2, lam, dtype=np.float64)[2] for lam in np.linspace(0, hi, 25)]
    assert np.all(np.diff(rss) >= -1e-9 * rss[-1])


@pytest.mark.parametrize("T", [1000, 4097])
@pytest.mark.parametrize("d,r", PAIRS + ((0.5, 0.2), (0.9, 0.9), (0.95, 0.0)))
def test_emulation_tracks_float64(T, d, r):
    y, _, _ = R2.planted2(7, T=T, d=d, r=r, sigma=SIGMA)
    g = DX.ar2_from_roots(d, r).astype(np.float32)
    t32, t64 = R2.tables(g[0], g[1], T), R2.tables(g[0], g[1], T, np.float64)
    for lam in (0.0, 0.5, 2.0):
        c, s, rss, n_pools = R2.oasis_ar2(y, g[0], g[1], lam, dtype=np.float32, tab=t32)
        c6, s6, rss6, n6 = R2.oasis_ar2(y, g[0], g[1], lam, dtype=np.float64, tab=t64)
        assert c.dtype == np.float32 and s.dtype == np.float32
        err = max(np.abs(c - c6).max(), np.abs(s - s6).max()) / np.abs(y).max()
        print("T", T, "roots", d, r, "lam", lam, "fp32 - float64 / max|y|", err, "pools", n_pools, n6)
        assert n_pools == n6
        assert err <= 4 * EMULATION_ERR2
        assert abs(rss - rss6) <= 1e-6 * rss6


# ---- the tables ----------------------------------------------------------------------------------------------------
def test_ar2_tables():
    T = 300
    for d, r in ((0.95, 0.5), (0.9, 0.3), (0.5, 0.25)):
        g1, g2 = np.float32(d + r), np.float32(-d * r)
        tab = DX.ar2_tables(g1, g2, T)
        assert tab.dtype == np.float32 and tab.shape == (3, T + 2)
        # the closed form on the roots of the fp32 pair
        g1d, g2d = float(g1), float(g2)
        root = np.sqrt(g1d * g1d + 4 * g2d)
        dd, rr = (g1d + root) / 2, (g1d - root) / 2
        j = np.arange(T + 1, dtype=np.float64)
        h = (dd ** (j + 1) - rr ** (j + 1)) / (dd - rr)
        live = h >= 1e-30
        assert tab[0, 0] == 0 and tab[0, 1] == 1
        assert np.abs(tab[0, 1:][live] / h[live] - 1).max() <= 1e-6
        assert np.abs(tab[1, 1:T + 1] / np.cumsum(h[:T] ** 2) - 1).max() <= 1e-6
        assert np.abs(tab[2, 2:T + 1] / np.cumsum(h[1:T] * h[:T - 1]) - 1).max() <= 1e-6
        assert tab[1, 0] == 0 and tab[2, 0] == 0 and tab[2, 1] == 0 and tab[1, 1] == 1
        assert tab[1, T + 1] == 0 and tab[2, T + 1] == 0
    # the double root: h_j = (j + 1) d^j
    h = DX.ar2_tables(1.0, -0.25, 40)[0]
    j = np.arange(41, dtype=np.float64)
    assert np.array_equal(h[1:], ((j + 1) * 0.5 ** j).astype(np.float32))
    # nothing denormal in H: entries below FLT_MIN are exactly 0, the sums stop growing
    tab = DX.ar2_tables(0.75, -0.125, 400)                     # roots 0.5 and 0.25
    tiny = np.finfo(np.float32).tiny
    assert np.all((tab[0] == 0) | (tab[0] >= tiny)) and tab[0, 1 + 125] > 0 and np.all(tab[0, 1 + 127:] == 0)
    assert tab[1, 400] == tab[1, 200] > 1 and tab[2, 400] == tab[2, 200] > 0
    # arrays of pairs: one set of three rows each, equal to the scalar call; g2 = 0 is the power table
    both = DX.ar2_tables(np.float32([1.45, 0.5]), np.float32([-0.475, 0.0]), 50)
    assert both.shape == (2, 3, 52)
    assert np.array_equal(both[0], DX.ar2_tables(np.float32(1.45), np.float32(-0.475), 50))
    assert np.array_equal(both[1, 0, 1:], DX.power_table(0.5, 50))
    assert np.array_equal(R2.tables(np.float32(1.45), np.float32(-0.475), 50), both[0])


def test_the_merge_identity_of_the_impulse_response():
    """h_{m+j} = h_m h_j + g2 h_{m-1} h_{j-1}: what makes N and M of two pools combine in O(1)."""
    g1, g2 = 1.45, -0.475
    h = R2.tables(g1, g2, 120, np.float64)[0]                  # h[i] = h_{i-1}
    m, j = np.meshgrid(np.arange(1, 60), np.arange(0, 60), indexing="ij")
    lhs = h[m + j + 1]
    rhs = h[m + 1] * h[j + 1] + g2 * h[m] * h[j]
    assert np.abs(lhs - rhs).max() <= 1e-14 * h.max()
    # and so the sums of a merged pool: N over m + l frames from the parts
    rng = np.random.default_rng(0)
    y = rng.standard_normal(30)
    mm, l = 11, 19
    n_top, m_top = h[1:l + 1] @ y[mm:], h[:l] @ y[mm:]
    assert h[1:31] @ y == pytest.approx(h[1:mm + 1] @ y[:mm] + h[mm + 1] * n_top + g2 * h[mm] * m_top, rel=1e-13)
    assert h[:30] @ y == pytest.approx(h[:mm] @ y[:mm] + h[mm] * n_top + g2 * h[mm - 1] * m_top, rel=1e-13)


def test_ar2_from_roots_and_time_constants():
    g = localmd_amd.ar2_from_roots(0.95, 0.5)
    assert g.shape == (2,) and g.dtype == np.float64
    assert np.array_equal(g, np.float32([1.45, -0.475]).astype(np.float64))
    many = localmd_amd.ar2_from_roots([0.95, 0.9, 0.5], [0.5, 0.0, 0.5])
    assert many.shape == (3, 2) and many[1, 1] == 0 and DX.ar2_violation(many[:, 0], many[:, 1]) is None
    # a double root stays admissible once rounded to fp32: r gives way by a few steps of 2^-12
    for d in (0.9, 0.3, 0.9999, 0.7071067811865476):
        g = localmd_amd.ar2_from_roots(d, d)
        assert DX.ar2_violation(g[0], g[1]) is None
        dh, rh = roots(g)
        assert abs(dh[0] - d) <= 2e-3 and 0 <= d - rh[0] <= 4e-3
    for bad in ((0.5, 0.6), (1.0, 0.5), (0.9, -0.1), (1.5, 0.2)):
        with pytest.raises(ValueError, match="roots"):
            localmd_amd.ar2_from_roots(*bad)
    g = localmd_amd.ar2_from_time_constants(0.05, 0.7, 30.0)
    want = localmd_amd.ar2_from_roots(np.exp(-1 / (0.7 * 30.0)), np.exp(-1 / (0.05 * 30.0)))
    assert np.array_equal(g, want)
    with pytest.raises(ValueError, match="tau_rise"):
        localmd_amd.ar2_from_time_constants(0.7, 0.05, 30.0)
    with pytest.raises(ValueError, match="frame_rate"):
        localmd_amd.ar2_from_time_constants(0.05, 0.7, 0.0)


# ---- the ceiling of the search ---------------------------------------------------------------------------------------
def test_lambda_ceiling_of_pairs():
    g = np.float32([[0.75, -0.125], [1.25, -0.375]])           # 1 - g1 > 0, and 1 - g1 < 0: the frame T - 2 sets no bound
    y = np.float32([[1.0, 3.0, 2.0, 0.5, 0.25], [1.0, 3.0, 2.0, 9.0, 0.0]])
    hi = DX.lambda_ceiling(y, g, np.float32([1.0, 0.0]))
    assert hi.dtype == np.float32
    assert hi[0] == np.float32(max(2.0 / 0.375, -0.5 / 0.25, -0.75)) and hi[1] == np.float32(3.0 / 0.125)
    assert DX.lambda_ceiling(np.float32([[2.0]]), np.float32([[1.45, -0.475]]), np.float32([0.5]))[0] == 1.5
    assert DX.lambda_ceiling(np.float32([[8.0, 1.0]]), np.float32([[0.75, -0.125]]), np.float32([0.0]))[0] == 32.0
    assert np.array_equal(DX.lambda_ceiling(-y, g, np.float32([0, 0])), [0, 0])
    # 1 - g1 <= 0 and the maximum at frame T - 2: no lam makes that sample <= 0, the last two frames pool to <= 0 from
    # (y[T-2] - b) + g1 (y[T-1] - b) on; at it c = 0, just below it the pool of the two frames is positive
    tail = np.float32([-1.0, -2.0, -1.0, 10.0, -1.0])
    top = DX.lambda_ceiling(tail[None], g[1:], np.float32([0.0]))[0]
    assert top == np.float32(10.0 - 1.25)
    for dtype in (np.float32, np.float64):
        assert not R2.oasis_ar2(tail, g[1, 0], g[1, 1], top, dtype=dtype)[0].any()
        c = R2.oasis_ar2(tail, g[1, 0], g[1, 1], np.nextafter(top, np.float32(0)), dtype=dtype)[0]
        assert c[-2] > 0 and c[-1] > 0 and not c[:-2].any()
    assert DX.lambda_ceiling(np.float32([[10.0, -1.0]]), g[1:], np.float32([0.0]))[0] == np.float32(8.75)      # T = 2
    # the AR(1) rule is untouched
    assert DX.lambda_ceiling(y[:1], np.float32([0.5]), np.float32([1.0]))[0] == 4.0
    # at the ceiling nothing is left, on planted traces, in both precisions
    for seed, (d, r) in enumerate(PAIRS):
        yk, _, _ = R2.planted2(40 + seed, T=400, d=d, r=r, sigma=SIGMA)
        g32 = DX.ar2_from_roots(d, r).astype(np.float32)
        top = DX.lambda_ceiling(yk[None], g32[None], np.float32([0.1]))[0]
        assert top > 0
        for dtype in (np.float32, np.float64):
            c, s, _, n_pools = R2.oasis_ar2(yk, g32[0], g32[1], top, 0.0, np.float32(0.1), dtype)
            assert not c.any() and not s.any()
    # just below the ceiling something is left when the frame that sets it is the last one, whose sample nothing follows
    # (after an earlier frame the samples that follow may still pool it away): T = 1, and a trace that ends on its maximum
    for yk in (np.float32([2.0]), np.float32([-1.0, -3.0, -2.0, -1.0, 4.0])):
        for g32 in g:
            top = DX.lambda_ceiling(yk[None], g32[None], np.float32([0.0]))[0]
            assert top == yk[-1]
            below = np.nextafter(top, np.float32(0))
            for dtype in (np.float32, np.float64):
                assert not R2.oasis_ar2(yk, g32[0], g32[1], top, dtype=dtype)[0].any()
                c = R2.oasis_ar2(yk, g32[0], g32[1], below, dtype=dtype)[0]
                assert c[-1] > 0 and not c[:-1].any()


# ---- the estimate --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,r", PAIRS)
def test_estimate_ar2_on_planted_traces(d, r):
    y = np.stack([R2.planted2(seed, T=10000, d=d, r=r, sigma=SIGMA)[0] for seed in (11, 12, 13, 14)])
    g = localmd_amd.estimate_ar2(y, SIGMA)
    assert g.shape == (4, 2) and g.dtype == np.float64
    assert np.array_equal(g, g.astype(np.float32).astype(np.float64)) and DX.ar2_violation(g[:, 0], g[:, 1]) is None
    dh, rh = roots(g)
    print("roots", d, r, "d^ - d", dh - d, "r^ - r", rh - r)
    assert np.abs(dh - d).max() <= 2 * ESTIMATE_ERR[(d, r)][0]
    assert np.abs(rh - r).max() <= 2 * ESTIMATE_ERR[(d, r)][1]
    assert np.array_equal(DX.estimate_ar2(y, [SIGMA] * 4, lags=10), g)


def test_estimate_ar2_complex_roots_and_clipping():
    rng = np.random.default_rng(5)
    t = np.arange(4000)
    # a damped oscillation has a complex pair: its real part twice (0.9 cos(0.3) = 0.86), a double root
    e = rng.standard_normal(4000)
    x = np.zeros(4000)
    for i in range(2, 4000):
        x[i] = 2 * 0.9 * np.cos(0.3) * x[i - 1] - 0.81 * x[i - 2] + e[i]
    g = DX.estimate_ar2(x[None], 0.0)
    dh, rh = roots(g)
    assert abs(dh[0] - 0.9 * np.cos(0.3)) <= 0.02 and 0 <= dh[0] - rh[0] <= 4e-3
    assert DX.ar2_violation(g[:, 0], g[:, 1]) is None
    # an alternating trace has a root at -1: clipped to 0, and the other one is next to 0
    alternating = np.where(t % 2 == 0, 1.0, -1.0) + 0.01 * rng.standard_normal(4000)
    g = DX.estimate_ar2(alternating[None], 0.01)
    assert 0 <= g[0, 0] <= 0.01 and g[0, 1] == 0
    # a slow sine has its roots at 1: clipped to 0.9999, and r gives way until fp32 holds an admissible pair
    slow = np.sin(2 * np.pi * t / 4000)
    g = DX.estimate_ar2(slow[None], 0.0)
    dh, rh = roots(g)
    assert abs(dh[0] - 0.9999) <= 1e-3 and DX.ar2_violation(g[:, 0], g[:, 1]) is None
    # white noise, and nothing at all
    white = DX.estimate_ar2(rng.standard_normal((8, 4000)), 1.0)
    assert white.shape == (8, 2) and DX.ar2_violation(white[:, 0], white[:, 1]) is None
    assert np.array_equal(DX.estimate_ar2(np.zeros((1, 100)), 1.0), [[0.0, 0.0]])
    with pytest.raises(ValueError, match="lags"):
        DX.estimate_ar2(np.zeros((1, 11)), 1.0)
    DX.estimate_ar2(np.zeros((1, 12)), 1.0)
    with pytest.raises(ValueError, match="lags"):
        DX.estimate_ar2(np.zeros((1, 100)), 1.0, lags=1)


# ---- argument checks (all before any device work: they raise without a device) -------------------------------------
@pytest.mark.parametrize("kwargs,match", [
    (dict(p=3), "p must be"), (dict(p=0), "p must be"), (dict(p="2"), "p must be"), (dict(p=True), "p must be"),
    (dict(p=2.5), "p must be"),
    (dict(p=2, g=0.9), "pair"), (dict(p=2, g=[0.9, 0.3, 0.1]), "pair"), (dict(p=2, g=np.zeros((3, 2))), "pair"),
    (dict(p=2, g="slow"), "pair"),
    (dict(p=2, g=(-0.1, 0.0)), "g1 >= 0"), (dict(p=2, g=(0.5, 0.1)), "g2 <= 0"),
    (dict(p=2, g=(1.0, -0.5)), "real roots"), (dict(p=2, g=(1.5, -0.5)), "1 - g1 - g2 > 0"),
    (dict(p=2, g=(1.0, 0.0)), "1 - g1 - g2 > 0"), (dict(p=2, g=(4.0, -4.0)), "g1 < 2"),
    (dict(p=2, g=(np.nan, 0.0)), "finite"), (dict(p=2, g=(1.8, np.float64(-0.81) * (1 + 1e-9))), "real roots"),
    (dict(p=2, g=[(1.45, -0.475), (1.0, -0.5)]), "real roots"),
    (dict(p=2, g=(1.45, -0.475), noise=0.0), "noise"), (dict(p=2, g=(1.45, -0.475), lam=-1.0), "lam"),
    (dict(p=2, g=(1.45, -0.475), max_workspace_bytes=24 * 300 - 1), "max_workspace_bytes"),
    (dict(p=1, g=[(0.9, 0.0), (0.9, 0.0)]), "g"),
])
def test_argument_errors(kwargs, match):
    y = np.zeros((2, 300), dtype=np.float32)
    with pytest.raises(ValueError, match=match):
        localmd_amd.deconvolve(y, **kwargs)


def test_trace_length_errors():
    with pytest.raises(ValueError, match="g="):
        localmd_amd.deconvolve(np.zeros((2, 11)), noise=1.0, p=2)
    with pytest.raises(ValueError, match="noise="):
        localmd_amd.deconvolve(np.zeros((2, 255)), g=(1.45, -0.475), p=2)


def test_checked_arguments_of_pairs():
    out = DX.check_arguments(np.arange(12).reshape(2, 6), (1.45, -0.475), [1, 2], None, 0.25, [0.5, -0.5], 5, 8, 1 << 20, p=2)
    y, g, noise, lam, s_min, b, rounds, points, cap = out
    assert g.shape == (2, 2) and g.dtype == np.float64 and np.array_equal(g, [[1.45, -0.475]] * 2)
    assert np.array_equal(noise, [1, 2]) and lam is None and np.array_equal(b, [0.5, -0.5])
    g = DX.check_arguments(np.zeros((2, 6)), [(1.45, -0.475), (0.5, 0.0)], 1.0, None, 0, 0, 5, 8, 1 << 20, p=2)[1]
    assert np.array_equal(g, [[1.45, -0.475], [0.5, 0.0]])
    # p = 1 by keyword is the call without it
    a = DX.check_arguments(np.zeros((2, 6)), 0.5, 1.0, None, 0, 0, 5, 8, 1 << 20)
    b = DX.check_arguments(np.zeros((2, 6)), 0.5, 1.0, None, 0, 0, 5, 8, 1 << 20, p=1)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


# ---- the plans -----------------------------------------------------------------------------------------------------
def test_launch_plan_of_pairs():
    T = 100
    one = 24 * T
    wave = 64 * one
    assert DX.workspace_bytes(T, 1, p=2) == one and DX.workspace_bytes(T, 65, p=2) == 65 * one
    assert DX.workspace_bytes(T, 7, p=2) == DX.workspace_bytes(T, 14)      # pmd_oasis_ar1_workspace_bytes(T, 2 n_prob)
    assert DX.launch_plan(130, T, wave, p=2) == [(0, 64), (64, 128), (128, 130)]
    assert DX.launch_plan(130, T, 3 * wave - 1, p=2) == [(0, 128), (128, 130)]
    assert DX.launch_plan(130, T, 1 << 30, p=2) == [(0, 130)]
    assert DX.launch_plan(20, T, 10 * one + one - 1, p=2) == [(0, 10), (10, 20)]
    assert DX.launch_plan(3, T, one, p=2) == [(0, 1), (1, 2), (2, 3)]
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        DX.launch_plan(1, T, one - 1, p=2)
    with pytest.raises(ValueError, match="p must be"):
        DX.launch_plan(1, T, one, p=3)


def test_deconvolve_device_bytes_of_pairs():
    K, T = 7, 1000
    resident = 12 * K * T + 12 * K * (T + 2)
    one = DX.deconvolve_device_bytes(K=K, T=T, problems=8 * K, max_workspace_bytes=1 << 30, p=2)
    assert one == resident + 24 * T * 56 + 40 * 56 + (1 << 20)
    capped = DX.deconvolve_device_bytes(K=100, T=T, problems=800, max_workspace_bytes=24 * T * 64 * 3, stats_bytes=5000, p=2)
    assert capped == 12 * 100 * T + 1200 * (T + 2) + 24 * T * 192 + 40 * 192 + 5000 + (1 << 20)
    with pytest.raises(ValueError):
        DX.deconvolve_device_bytes(K=K, T=T, problems=8 * K, max_workspace_bytes=24 * T - 1, p=2)


def test_the_plans_of_the_first_order_are_unchanged():
    T = 100
    for n, cap in ((130, 64 * 12 * T), (130, 3 * 64 * 12 * T - 1), (20, 11 * 12 * T - 1), (3, 12 * T), (64, 1 << 30)):
        assert DX.launch_plan(n, T, cap, p=1) == DX.launch_plan(n, T, cap)
    assert DX.launch_plan(130, T, 64 * 12 * T) == [(0, 64), (64, 128), (128, 130)]
    assert DX.workspace_bytes(T, 65, p=1) == DX.workspace_bytes(T, 65) == 65 * 12 * T
    for kw in (dict(K=7, T=1000, problems=56, max_workspace_bytes=1 << 30),
               dict(K=100, T=1000, problems=800, max_workspace_bytes=12 * 1000 * 64 * 3, stats_bytes=5000)):
        assert DX.deconvolve_device_bytes(p=1, **kw) == DX.deconvolve_device_bytes(**kw)
    assert DX.deconvolve_device_bytes(K=7, T=1000, problems=56, max_workspace_bytes=1 << 30) == \
        12 * 7 * 1000 + 4 * 7 * 1001 + 12 * 1000 * 56 + 36 * 56 + (1 << 20)
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        DX.launch_plan(1, T, 12 * T - 1, p=1)


# ---- the planted property and the onset ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_run(seed, rate):
    y, times, amps = R2.planted2(seed, d=0.95, r=0.5, sigma=SIGMA, rate=rate)
    return R2.deconvolve_ref2(y[None], DX.ar2_from_roots(0.95, 0.5), SIGMA)


@pytest.mark.parametrize("seed,rate", PLANTED)
def test_planted_events_are_found(seed, rate):
    """The bounds of tests/test_deconvolve_host.py on the AR(2) traces: the search ends within 0.1 % below the noise
    target, nine in ten of the events above 4 sigma (peak height) have more than a third of that in spikes within one
    frame (a unit-peak event is a spike of 1 / max h = 0.60 for these roots), and no spike above 3 sigma lies elsewhere."""
    _, times, amps = R2.planted2(seed, d=0.95, r=0.5, sigma=SIGMA, rate=rate)
    r = planted_run(seed, rate)
    ratio = r["rss"][0] / r["target"][0]
    hit, big, false_pos = R1.planted_property(r["spikes"][0], times, amps, SIGMA)
    print("seed", seed, "rss / target", ratio, "lam", r["lam"][0], "found", hit, "of", big, "false positives", false_pos)
    assert 0.999 <= ratio <= 1.0 and r["evaluations"][0] == 2 + 5 * 8 + 1 and r["lam"][0] > 0
    assert big >= 8 and hit >= 0.9 * big
    assert false_pos == 0


@pytest.mark.parametrize("seed,rate", PLANTED)
def test_the_rise_is_not_explained_by_early_spikes(seed, rate):
    """On a planted rise the spikes within one frame of the events above 4 sigma carry a larger share of all spike mass
    with the AR(2) model than with the AR(1) model at its own estimate_decay, which spends mass on the frames of the
    rise and on re-fitting the slower peak."""
    y, times, amps = R2.planted2(seed, d=0.95, r=0.5, sigma=SIGMA, rate=rate)
    s2 = planted_run(seed, rate)["spikes"][0].astype(np.float64)
    s1 = R1.deconvolve_ref(y[None], DX.estimate_decay(y[None], SIGMA), SIGMA)["spikes"][0].astype(np.float64)
    near = np.zeros(len(y), dtype=bool)
    for t, a in zip(times, amps):
        if a > 4 * SIGMA:
            near[max(0, t - 1):t + 2] = True
    share2, share1 = s2[near].sum() / s2.sum(), s1[near].sum() / s1.sum()
    print("seed", seed, "share of the spike mass at the events: p = 2", share2, "p = 1", share1)
    assert share2 > share1
