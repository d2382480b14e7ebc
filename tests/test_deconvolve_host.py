"""Host side of localmd_amd.deconvolve (no device): the NumPy restatement of the OASIS AR(1) solver (tests/oasis_ref.py)
against scipy's NNLS and against itself in fp32, the penalty search as a pure function of ``solve`` driven by that
emulation, the decay estimate, the launch and memory plans, the argument checks, and the planted-event property."""
import functools
import importlib

import numpy as np
import pytest

import localmd_amd
from tests import oasis_ref as R

DX = importlib.import_module("localmd_amd.deconvolve")     # the module: the package exports the function under the same name

SIGMA = 0.3
PLANTED = ((1, 0.015), (2, 0.02), (3, 0.01))      # (seed, event rate) of the planted traces: g = 0.95, T = 3000
# fp32 emulation against the float64 form on the inputs of test_emulation_tracks_float64, as a fraction of max |y|:
# the largest value measured over its 24 cases is 4.18e-7 (T = 4097, g = 0.5, lam = 0.5); the bound is four times
# that, the rule of tests/test_gpu_demix.py.
EMULATION_ERR = 4.18e-7


@functools.lru_cache(maxsize=None)
def planted_run(seed, rate, dtype_name):
    y, times, amps = R.planted(seed, rate=rate)
    return R.deconvolve_ref(y[None], 0.95, SIGMA, dtype=getattr(np, dtype_name))


# ---- the solver's arithmetic ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [60, 200])
@pytest.mark.parametrize("g", [0.0, 0.5, 0.9, 0.95])
@pytest.mark.parametrize("lam", [0.0, 0.3])
def test_float64_form_is_the_nnls_solution(T, g, lam):
    y, _, _ = R.planted(T + int(100 * g), T=T, g=g if g else 0.5, sigma=SIGMA, rate=0.05)
    c, s, rss, n_pools = R.oasis_ar1(y, g, lam, dtype=np.float64)
    cn, sn = R.nnls_ref(y, g, lam)
    err = max(np.abs(c - cn).max(), np.abs(s[1:] - sn[1:]).max()) / np.abs(y).max()
    print("T", T, "g", g, "lam", lam, "distance to nnls / max|y|", err)
    assert err <= 1e-6
    assert s[0] == 0 and np.all(s >= 0) and np.all(c >= 0)
    d = y.astype(np.float64) - c
    assert rss == pytest.approx(float(d @ d), rel=1e-12)
    assert 1 + np.count_nonzero(s) <= n_pools <= T


@pytest.mark.parametrize("T", [1000, 4097])
@pytest.mark.parametrize("g", [0.5, 0.9, 0.95, 0.995])
def test_emulation_tracks_float64(T, g):
    y, _, _ = R.planted(7, T=T, g=g, sigma=SIGMA)
    g32 = np.float32(g)
    for lam in (0.0, 0.5, 2.0):
        c, s, rss, n_pools = R.oasis_ar1(y, g32, lam, dtype=np.float32)
        c6, s6, rss6, n6 = R.oasis_ar1(y, g32, lam, dtype=np.float64)
        assert c.dtype == np.float32 and s.dtype == np.float32
        err = max(np.abs(c - c6).max(), np.abs(s - s6).max()) / np.abs(y).max()
        print("T", T, "g", g, "lam", lam, "fp32 - float64 / max|y|", err, "pools", n_pools, n6)
        assert err <= 4 * EMULATION_ERR
        assert n_pools == n6
        assert abs(rss - rss6) <= 1e-6 * rss6


def test_power_table():
    pw = DX.power_table(0.5, 200)
    assert pw.dtype == np.float32 and pw.shape == (201,)
    assert pw[0] == 1 and pw[126] == np.float32(2.0 ** -126) and np.all(pw[127:] == 0)     # nothing denormal
    g32 = np.float32(0.95)
    pw = DX.power_table([0.95, 0.0], 50)
    assert pw.shape == (2, 51)
    assert np.array_equal(pw[0], (np.float64(g32) ** np.arange(51)).astype(np.float32))
    assert pw[1, 0] == 1 and np.all(pw[1, 1:] == 0)
    assert np.array_equal(R.power_table(0.95, 50), pw[0])


# ---- the search ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,rate", PLANTED)
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_search_meets_the_noise_constraint(seed, rate, dtype_name):
    r = planted_run(seed, rate, dtype_name)
    ratio = r["rss"][0] / r["target"][0]
    print("seed", seed, dtype_name, "rss / target", ratio, "lam", r["lam"][0], "evaluations", r["evaluations"][0])
    assert 0.999 <= ratio <= 1.0
    assert r["evaluations"][0] == 2 + 5 * 8 + 1
    assert r["lam"].dtype == np.float32 and r["lam"][0] > 0


def test_search_first_exit_rss_at_zero_already_at_the_target():
    y, _, _ = R.planted(1, T=400)
    r = R.deconvolve_ref(y[None], 0.95, 1e-3)        # no penalty can bring the residual down to this noise level
    assert r["lam"][0] == 0 and r["evaluations"][0] == 3
    assert r["rss"][0] >= r["target"][0]


def test_search_second_exit_a_trace_of_noise_below_sigma():
    y = (0.1 * np.random.default_rng(4).standard_normal(500)).astype(np.float32)
    r = R.deconvolve_ref(y[None], 0.9, 1.0)
    hi = DX.lambda_ceiling(y[None], np.float32([0.9]), np.float32([0]))
    assert r["lam"][0] == hi[0] > 0 and r["evaluations"][0] == 3
    assert not r["calcium"].any() and not r["spikes"].any()
    assert r["rss"][0] == pytest.approx(float(y.astype(np.float64) @ y.astype(np.float64)), rel=1e-12)


def test_search_grid_selection_and_collapsed_bracket():
    """A step function as rss: lam qualifies iff it is at most ``edge``.  The search has to end exactly on the edge, its
    bracket collapses to two neighbouring fp32 numbers and the trace drops out of the later rounds; a second trace with
    another edge goes on alone, and every batch names only traces still searching."""
    edge = np.float32([0.3, 1.7])
    calls = []

    def solve(idx, lam):
        assert lam.dtype == np.float32 and len(idx) == len(lam)
        calls.append(np.unique(idx).tolist())
        return np.where(lam <= edge[idx], 0.5, 2.0)

    lam, ev = DX.search_lambda(solve, np.array([1.0, 1.0]), np.float32([1.0, 2.0 ** 20]), rounds=40, points=8)
    assert np.array_equal(lam, edge)
    assert calls[0] == [0, 1] and calls[-1] == [1] and [0, 1] in calls[1:]
    assert ev[0] < ev[1] < 2 + 40 * 8 and (ev[0] - 2) % 8 == 0
    # one round of three points on [0, 4]: candidates 1, 2, 3; the largest qualifying entry is taken even when a smaller
    # one does not qualify (lo always does)
    seen = []

    def solve2(idx, lam):
        seen.append(lam.copy())
        return np.where(np.isin(lam, [0.0, 2.0]), 0.5, 2.0)

    lam, ev = DX.search_lambda(solve2, np.array([1.0]), np.float32([4.0]), rounds=1, points=3)
    assert np.array_equal(seen[1], np.float32([1, 2, 3])) and lam[0] == 2 and ev[0] == 5


def test_launch_plan():
    T = 100
    one = 12 * T
    wave = 64 * one
    assert DX.workspace_bytes(T, 1) == one and DX.workspace_bytes(T, 65) == 65 * one
    assert DX.launch_plan(130, T, wave) == [(0, 64), (64, 128), (128, 130)]
    assert DX.launch_plan(130, T, 3 * wave - 1) == [(0, 128), (128, 130)]       # whole waves beyond the first
    assert DX.launch_plan(130, T, 1 << 30) == [(0, 130)]
    assert DX.launch_plan(64, T, wave) == [(0, 64)]
    assert DX.launch_plan(20, T, 10 * one + one - 1) == [(0, 10), (10, 20)]      # below a wave: problem by problem
    assert DX.launch_plan(3, T, one) == [(0, 1), (1, 2), (2, 3)]
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        DX.launch_plan(1, T, one - 1)


def test_deconvolve_device_bytes():
    K, T = 7, 1000
    resident = 12 * K * T + 4 * K * (T + 1)
    one = DX.deconvolve_device_bytes(K=K, T=T, problems=8 * K, max_workspace_bytes=1 << 30)
    assert one == resident + 12 * T * 56 + 36 * 56 + (1 << 20)
    big = DX.deconvolve_device_bytes(K=100, T=T, problems=800, max_workspace_bytes=1 << 30, stats_bytes=5000)
    assert big == 12 * 100 * T + 400 * (T + 1) + 12 * T * 800 + 36 * 800 + 5000 + (1 << 20)
    capped = DX.deconvolve_device_bytes(K=100, T=T, problems=800, max_workspace_bytes=12 * T * 64 * 3)
    assert capped == 12 * 100 * T + 400 * (T + 1) + 12 * T * 192 + 36 * 192 + (1 << 20)
    # the part that grows with T: resident terms and the (capped) stacks
    with pytest.raises(ValueError):
        DX.deconvolve_device_bytes(K=K, T=T, problems=8 * K, max_workspace_bytes=100)
    DX.check_fit(one, one)
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        DX.check_fit(one, one - 1)


# ---- the estimates -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,T,tol", [(0.95, 10000, 0.02), (0.9, 10000, 0.02), (0.8, 10000, 0.05), (0.9, 2048, 0.035)])
def test_estimate_decay_on_planted_traces(g, T, tol):
    y = np.stack([R.planted(seed, T=T, g=g, sigma=SIGMA)[0] for seed in (11, 12, 13)])
    est = DX.estimate_decay(y, SIGMA)
    print("g", g, "T", T, "estimate - g", est - g)
    assert est.shape == (3,) and est.dtype == np.float64
    assert np.all(np.abs(est - g) <= tol)
    assert np.array_equal(DX.estimate_decay(y, [SIGMA] * 3), est)


def test_estimate_decay_clips():
    rng = np.random.default_rng(5)
    white = DX.estimate_decay(rng.standard_normal((8, 4000)), 1.0)
    assert np.all((white >= 0) & (white <= 0.9999))
    t = np.arange(4000)
    alternating = np.where(t % 2 == 0, 1.0, -1.0) + 0.01 * rng.standard_normal(4000)
    assert DX.estimate_decay(alternating[None], 0.01)[0] == 0.0
    slow = np.sin(2 * np.pi * t / 4000)               # xc[tau] = xc[0] to 1e-4, and half of xc[0] is declared noise
    assert DX.estimate_decay(slow[None], 0.5)[0] == 0.9999
    assert DX.estimate_decay(np.zeros((1, 100)), 1.0)[0] == 0.0
    with pytest.raises(ValueError):
        DX.estimate_decay(np.zeros((1, 5)), 1.0)


def test_lambda_ceiling():
    y = np.float32([[1.0, 3.0, 2.0, 5.0], [-1.0, -2.0, -3.0, -0.5]])
    hi = DX.lambda_ceiling(y, np.float32([0.5, 0.5]), np.float32([1.0, 0.0]))
    assert hi.dtype == np.float32 and np.array_equal(hi, np.float32([4.0, 0.0]))
    assert DX.lambda_ceiling(np.float32([[2.0]]), np.float32([0.9]), np.float32([0.5]))[0] == 1.5
    # at the ceiling nothing is left
    c, s, _, n_pools = R.oasis_ar1(y[0], 0.5, hi[0], 0.0, 1.0)
    assert not c.any() and not s.any()


# ---- argument checks (all before any device work: they raise without a device) -------------------------------------
@pytest.mark.parametrize("kwargs,match", [
    (dict(g=1.0), "g"), (dict(g=-0.1), "g"), (dict(g=[0.5, 0.5, 0.5]), "g"), (dict(g="fast"), "g"),
    (dict(noise=0.0), "noise"), (dict(noise=-1.0), "noise"), (dict(noise=np.nan), "noise"),
    (dict(lam=-1.0), "lam"), (dict(lam=np.inf), "lam"), (dict(s_min=-0.5), "s_min"), (dict(baseline=np.inf), "baseline"),
    (dict(search_rounds=0), "search_rounds"), (dict(search_points=0), "search_points"), (dict(search_points=2.5), "search_points"),
    (dict(max_workspace_bytes=3599), "max_workspace_bytes"), (dict(max_workspace_bytes=0), "max_workspace_bytes"),
])
def test_argument_errors(kwargs, match):
    y = np.zeros((2, 300), dtype=np.float32)
    with pytest.raises(ValueError, match=match):
        localmd_amd.deconvolve(y, **kwargs)


def test_trace_errors():
    with pytest.raises(ValueError, match="traces"):
        localmd_amd.deconvolve(np.zeros(300))
    with pytest.raises(ValueError, match="traces"):
        localmd_amd.deconvolve(np.zeros((0, 300)))
    with pytest.raises(ValueError, match="traces"):
        localmd_amd.deconvolve(np.zeros((2, 300), dtype=complex))
    for bad in (np.nan, np.inf, -np.inf, 1e39):
        y = np.zeros((2, 300))
        y[1, 17] = bad
        with pytest.raises(ValueError, match="finite"):
            localmd_amd.deconvolve(y, noise=1.0, g=0.9)
    with pytest.raises(ValueError, match="noise="):
        localmd_amd.deconvolve(np.zeros((2, 255)), g=0.9)
    with pytest.raises(ValueError, match="g="):
        localmd_amd.deconvolve(np.zeros((2, 5)), noise=1.0)


def test_checked_arguments_are_per_trace():
    y, g, noise, lam, s_min, b, rounds, points, cap = DX.check_arguments(
        np.arange(12).reshape(2, 6), 0.5, [1, 2], None, 0.25, [0.5, -0.5], 5, 8, 1 << 20)
    assert y.dtype == np.float32 and y.shape == (2, 6)
    assert np.array_equal(g, [0.5, 0.5]) and np.array_equal(noise, [1, 2]) and lam is None
    assert s_min.dtype == np.float32 and np.array_equal(s_min, [0.25, 0.25])
    assert b.dtype == np.float32 and np.array_equal(b, [0.5, -0.5])
    assert (rounds, points, cap) == (5, 8, 1 << 20)


# ---- the launch sequence (a context that records its calls; no device, no library) ----------------------------------
def test_solver_launch_sequence():
    """_Solver.solve on K = 3 traces of T = 7 frames with 5 problems, for both orders, under a cap that holds every
    problem and under one that holds two: per launch the entry point, n_prob, the table's leading dimension, the ``par``
    rows read back through the pointer (fp32, in the entry point's column order), the table rows (p = 1: the tensor of
    the columns itself, no second upload; p = 2: three times the columns), the workspace of the largest launch, and
    where in C and S the launch writes."""
    import ctypes
    import types
    import torch

    T, K, n = 7, 3, 5
    idx, lam = np.int64([2, 0, 1, 1, 2]), np.float32([0.0, 0.5, 1.0, 1.5, 2.0])
    s_min, b = np.float32([0.0, 0.1, 0.2]), np.float32([0.3, 0.0, -0.3])
    g1 = np.float32([0.5, 0.9, 0.95])
    g2 = np.float32([[1.45, -0.475], [0.75, -0.125], [0.9, 0.0]])
    par1 = np.stack([g1[idx], lam, s_min[idx], b[idx]], axis=1)
    par2 = np.stack([g2[idx, 0], g2[idx, 1], lam, s_min[idx], b[idx]], axis=1)

    def read(p, ctype, count):
        return np.ctypeslib.as_array((ctype * count).from_address(p.value)).copy()

    for p, entry, g, par, ldtab, rows, pool in ((1, "pmd_oasis_ar1", g1, par1, 8, 1, 12),
                                                (2, "pmd_oasis_ar2", g2, par2, 9, 3, 24)):
        for cap, plan in ((1 << 30, [(0, 5)]), (2 * pool * T, [(0, 2), (2, 4), (4, 5)])):
            calls = []

            def call(name, *a):
                (Y_, ldy, T_, n_prob, col, pr, row, tab, ld, C_, ldc, S_, lds, r, npl, ws, ws_bytes) = a
                width = par.shape[1]
                calls.append(dict(
                    name=name, ints=(ldy, T_, n_prob, ld, ldc, lds, ws_bytes), col=read(col, ctypes.c_int32, n_prob),
                    par=read(pr, ctypes.c_float, n_prob * width).reshape(n_prob, width), same=row.value == col.value,
                    row=read(row, ctypes.c_int32, n_prob),
                    ptrs=(Y_.value, tab.value, C_ and C_.value, S_ and S_.value, ws.value)))
                ctypes.memmove(r.value, (100.0 * len(calls) + np.arange(n_prob, dtype=np.float64)).ctypes.data, 8 * n_prob)
                if npl.value:
                    ctypes.memmove(npl.value, (10 * len(calls) + np.arange(n_prob, dtype=np.int32)).ctypes.data, 4 * n_prob)

            ctx = types.SimpleNamespace(device=torch.device("cpu"), call=call)
            Y = torch.zeros((T, K), dtype=torch.float32)
            solver = DX._Solver(ctx, Y, g, s_min, b, cap, n, p)
            C, S = torch.zeros((T, n), dtype=torch.float32), torch.zeros((T, n), dtype=torch.float32)
            rss, n_pools = solver.solve(idx, lam, C, S, pools=True)
            largest = max(p1 - p0 for p0, p1 in plan)
            assert [c["name"] for c in calls] == [entry] * len(plan)
            want_rss, want_pools = [], []
            for k, (c, (p0, p1)) in enumerate(zip(calls, plan)):
                assert c["ints"] == (K, T, p1 - p0, ldtab, n, n, pool * T * largest), (p, cap, k)
                assert np.array_equal(c["col"], idx[p0:p1])
                assert c["par"].dtype == np.float32 and np.array_equal(c["par"], par[p0:p1])
                assert c["same"] == (p == 1) and np.array_equal(c["row"], rows * idx[p0:p1])
                assert c["ptrs"] == (Y.data_ptr(), solver.pw.data_ptr(), C.data_ptr() + 4 * p0, S.data_ptr() + 4 * p0,
                                     solver.ws.data_ptr())
                want_rss += list(100.0 * (k + 1) + np.arange(p1 - p0))
                want_pools += list(10 * (k + 1) + np.arange(p1 - p0))
            assert tuple(solver.pw.shape) == (rows * K, ldtab) and solver.ws.numel() == pool * T * largest
            assert np.array_equal(rss, want_rss) and np.array_equal(n_pools, want_pools)
            calls.clear()                                  # without C, S and n_pools: null pointers, the same launches
            solver.solve(idx, lam)
            assert [c["ints"][2] for c in calls] == [p1 - p0 for p0, p1 in plan]
            assert all(c["ptrs"][2:4] == (None, None) for c in calls)


# ---- the planted property ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,rate", PLANTED)
def test_planted_events_are_found(seed, rate):
    _, times, amps = R.planted(seed, rate=rate)
    r = planted_run(seed, rate, "float64")
    hit, big, false_pos = R.planted_property(r["spikes"][0], times, amps, SIGMA)
    print("seed", seed, "events above 4 sigma found", hit, "of", big, "false positives", false_pos)
    assert big >= 8 and hit >= 0.9 * big
    assert false_pos == 0
