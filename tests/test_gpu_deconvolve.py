"""Spike inference on the GPU (localmd_amd.deconvolve, csrc/oasis.hip): pmd_oasis_ar1 through the C ABI bit for bit
against its NumPy emulation (tests/oasis_ref.py) over the sizes where the mapping changes (one lane, a wave less one, a
wave, a wave and one, two waves and two), special traces, invariance over the requested outputs, the split into calls and
the position of a problem, and the error codes; deconvolve end to end against the package's own search driven by the
emulation; the planted-event property; and the growth of device memory with the trace length."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import localmd_amd
from tests import oasis_device as OD
from tests import oasis_ref as R
from tests import prep_ref
from tests.device_util import P, _t, dev as _dev

DX = importlib.import_module("localmd_amd.deconvolve")     # the module: the package exports the function under the same name

pytestmark = pytest.mark.gpu

PMD_ERR_ARG, PMD_ERR_WORKSPACE = -2, -3
SIGMA = 0.3
PLANTED = ((1, 0.015), (2, 0.02), (3, 0.01))      # the seeds and rates of tests/test_deconvolve_host.py
SIGMA_RTOL = 4 * 2.02e-7                          # pmd_stats against float64: the bound of tests/test_gpu_prep_stage.py
GS = (0.0, 0.5, 0.95, 0.999)
_bits, _assert_same, _assert_result = OD.bits, OD.assert_same, OD.assert_result
_device = functools.partial(OD.launch, OD.AR1)     # pmd_oasis_ar1: (ctx, Y, col, par, pw_row, pw, want=, pad=)


def _ar_traces(seed, T, K):
    """(T, K) float32: column k an AR(1) trace with the decay GS[k % 4], sparse events and noise."""
    rng = np.random.default_rng(seed)
    s = (rng.random((T, K)) < 0.08) * rng.uniform(0.5, 2.0, (T, K))
    c = np.zeros((T, K))
    for t in range(T):
        c[t] = (c[t - 1] * np.array([GS[k % 4] for k in range(K)]) if t else 0.0) + s[t]
    return (c + SIGMA * rng.standard_normal((T, K))).astype(np.float32)


def _problems(seed, n_prob, K):
    """col (repeats, no order), par = (g of the column, lam, s_min, b): every third problem has lam = 0, the others a
    positive one; s_min > 0 and b != 0 on a part of them."""
    rng = np.random.default_rng(seed)
    col = rng.integers(0, K, n_prob).astype(np.int32)
    if n_prob >= K:
        col[:K] = rng.permutation(K)
    par = np.zeros((n_prob, 4), dtype=np.float32)
    par[:, 0] = [GS[c % 4] for c in col]
    par[:, 1] = np.where(np.arange(n_prob) % 3 == 0, 0.0, rng.uniform(0.1, 1.5, n_prob))
    par[:, 2] = np.where(rng.random(n_prob) < 0.4, rng.uniform(0.05, 0.4, n_prob), 0.0)
    par[:, 3] = np.where(rng.random(n_prob) < 0.5, rng.uniform(-0.3, 0.3, n_prob), 0.0)
    return col, par


def _emulate(Y, col, par, pw_row, pw):
    """(C (T, n), S (T, n), rss (n,), n_pools (n,)) of the problems by the fp32 emulation; equal problems are solved once."""
    T, n = Y.shape[0], len(col)
    Ce, Se = np.zeros((T, n), dtype=np.float32), np.zeros((T, n), dtype=np.float32)
    rss, npl, seen = np.zeros(n), np.zeros(n, dtype=np.int32), {}
    for p in range(n):
        key = (int(col[p]), int(pw_row[p]), par[p].tobytes())
        if key not in seen:
            seen[key] = R.oasis_ar1(Y[:, col[p]], par[p, 0], par[p, 1], par[p, 2], par[p, 3], np.float32, pw[pw_row[p]])
        Ce[:, p], Se[:, p], rss[p], npl[p] = seen[key]
    return Ce, Se, rss, npl


@functools.lru_cache(maxsize=None)
def _case(T, n_prob):
    K = 9
    Y = _ar_traces(100 + T, T, K)
    col, par = _problems(T * 1000 + n_prob, n_prob, K)
    pw = DX.power_table([GS[k % 4] for k in range(K)], T)
    return Y, col, par, pw, _emulate(Y, col, par, col, pw)


# ---- pmd_oasis_ar1 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_prob", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("T", [1, 2, 3, 65, 257])
def test_oasis_bits(gpu_ctx, T, n_prob):
    Y, col, par, pw, ref = _case(T, n_prob)
    got = _device(gpu_ctx, Y, col, par, col, pw, pad=(3, 2, 5))
    _assert_same(got, ref)
    assert np.all(got["S"][0] == 0) and np.all(got["S"] >= 0) and np.all(got["C"] >= 0)


def test_oasis_bits_long(gpu_ctx):
    Y, col, par, pw, ref = _case(1500, 20)
    _assert_same(_device(gpu_ctx, Y, col, par, col, pw), ref)
    assert ref[3].min() >= 1 and ref[3].max() > 100


def test_oasis_special_traces(gpu_ctx):
    T = 300
    t = np.arange(T)
    rng = np.random.default_rng(8)
    half = DX.power_table(0.5, T)
    cols = {
        "increasing": 0.1 + 0.1 * t,                               # no merge: T pools
        "decreasing": 10.0 * 0.4 ** t - 1e-3,                      # every frame merges: one pool, back to frame 0
        "powers": np.where(t < 127, half[:T], 1.0 + t),            # y = pw while pw > 0: ties do not merge
        "negative": -1.0 - rng.random(T),                          # c = 0
        "long_pool": np.where(t == 0, 5.0, np.where(t < 200, -1.0, rng.random(T))),   # a pool of 200 frames: pw = 0
        "denormal": 1e-38 * rng.standard_normal(T),
    }
    names = list(cols)
    Y = np.stack([cols[k] for k in names], axis=1).astype(np.float32)
    col = np.arange(len(names), dtype=np.int32)
    par = np.zeros((len(names), 4), dtype=np.float32)
    par[:, 0] = 0.5
    par[names.index("denormal"), 0] = 0.95
    pw = np.stack([half, DX.power_table(0.95, T)])
    pw_row = (par[:, 0] == np.float32(0.95)).astype(np.int32)
    ref = _emulate(Y, col, par, pw_row, pw)
    got = _device(gpu_ctx, Y, col, par, pw_row, pw)
    _assert_same(got, ref)
    n = dict(zip(names, got["N"]))
    assert n["increasing"] == T and n["decreasing"] == 1 and n["powers"] == T
    assert not got["C"][:, names.index("negative")].any()
    assert np.all(got["C"][127:200, names.index("long_pool")] == 0) and got["C"][126, names.index("long_pool")] > 0
    d = got["C"][:, names.index("denormal")]
    assert np.any((d > 0) & (d < np.finfo(np.float32).tiny))     # denormals are kept


def test_oasis_nan_and_inf_samples(gpu_ctx):
    """One NaN, +inf or -inf sample: the call returns and gives what the stated arithmetic gives (a NaN never compares
    true, so it never merges and its pool is filled with 0; an infinite pool value spreads as the formulas say).  The
    emulation is compared value for value with NaN equal to NaN: the sign and payload of a NaN are not part of the
    statement."""
    T = 120
    base = _ar_traces(5, T, 3)
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        base[40, k] = bad
    col = np.arange(3, dtype=np.int32)
    par = np.float32([[0.5, 0.2, 0, 0], [0.5, 0.2, 0, 0], [0.5, 0.2, 0, 0]])
    pw = DX.power_table([0.5], T)
    pw_row = np.zeros(3, dtype=np.int32)
    Ce, Se, rss, npl = _emulate(base, col, par, pw_row, pw)
    got = _device(gpu_ctx, base, col, par, pw_row, pw)
    np.testing.assert_array_equal(got["C"], Ce)
    np.testing.assert_array_equal(got["S"], Se)
    np.testing.assert_array_equal(got["R"], rss)
    assert np.array_equal(got["N"], npl)
    assert got["C"][40, 0] == 0 and np.isnan(got["R"][0])
    assert np.array_equal(_bits(got["C"][:39]), _bits(Ce[:39]))


def test_oasis_bits_do_not_depend_on_outputs_split_or_position(gpu_ctx):
    Y, col, par, pw, ref = _case(257, 130)
    ctx = gpu_ctx
    for want in ("R", "N", "C", "S", "RN", "CS", "SR"):
        _assert_same(_device(ctx, Y, col, par, col, pw, want=want), ref, want)
    # two calls: problems 0 .. 69 and 70 .. 129
    for sl in (slice(0, 70), slice(70, 130)):
        part = tuple(r[..., sl] for r in ref)
        _assert_same(_device(ctx, Y, col[sl], par[sl], col[sl], pw), part)
    # the problems of one call embedded among others, in another order
    rng = np.random.default_rng(3)
    pick = rng.permutation(130)[:40]
    other_col, other_par = _problems(77, 100, Y.shape[1])
    where = np.sort(rng.choice(140, 40, replace=False))
    col2, par2 = np.zeros(140, dtype=np.int32), np.zeros((140, 4), dtype=np.float32)
    mask = np.zeros(140, dtype=bool)
    mask[where] = True
    col2[mask], par2[mask] = col[pick], par[pick]
    col2[~mask], par2[~mask] = other_col, other_par
    got = _device(ctx, Y, col2, par2, col2, pw, pad=(1, 0, 7))
    sub = {k: v[..., where] for k, v in got.items()}
    _assert_same(sub, tuple(r[..., pick] for r in ref))


def test_oasis_rejects_bad_arguments(gpu_ctx):
    torch, ctx = _t(), gpu_ctx
    T, K, n = 20, 3, 5
    Y = _dev(ctx, _ar_traces(1, T, K), np.float32)
    col = _dev(ctx, np.arange(n) % K, np.int32)
    par = _dev(ctx, np.tile(np.float32([0.5, 0.1, 0, 0]), (n, 1)), np.float32)
    row = _dev(ctx, np.zeros(n), np.int32)
    pw = _dev(ctx, DX.power_table([0.5], T), np.float32)
    Cd = torch.full((T, n), float("nan"), dtype=torch.float32, device=ctx.device)
    Sd = torch.full((T, n), float("nan"), dtype=torch.float32, device=ctx.device)
    rd = torch.full((n,), float("nan"), dtype=torch.float64, device=ctx.device)
    nd = torch.full((n,), -1, dtype=torch.int32, device=ctx.device)
    nbytes = ctx.lib.pmd_oasis_ar1_workspace_bytes(T, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=ctx.device)
    assert ctx.lib.pmd_oasis_ar1_workspace_bytes(0, n) == 0 and ctx.lib.pmd_oasis_ar1_workspace_bytes(T, 0) == 0
    good = dict(Y=P(Y), ldy=K, T=T, n=n, col=P(col), par=P(par), row=P(row), pw=P(pw), ldpw=T + 1, C=P(Cd), ldc=n, S=P(Sd),
                lds=n, rss=P(rd), np_=P(nd), ws=P(ws), wsb=nbytes)
    null = C.c_void_p(0)

    def rc(**change):
        a = dict(good, **change)
        return ctx.lib.pmd_oasis_ar1(ctx.handle, a["Y"], a["ldy"], a["T"], a["n"], a["col"], a["par"], a["row"], a["pw"],
                                     a["ldpw"], a["C"], a["ldc"], a["S"], a["lds"], a["rss"], a["np_"], a["ws"], a["wsb"])

    for change in (dict(T=0), dict(T=-3), dict(n=0), dict(ldy=0), dict(ldpw=T), dict(ldc=n - 1), dict(lds=n - 1),
                   dict(Y=null), dict(col=null), dict(par=null), dict(row=null), dict(pw=null),
                   dict(C=null, S=null, rss=null, np_=null)):
        assert rc(**change) == PMD_ERR_ARG, change
    for change in (dict(wsb=nbytes - 1), dict(ws=null)):
        assert rc(**change) == PMD_ERR_WORKSPACE, change
    assert ctx.lib.pmd_oasis_ar1(None, *[good[k] for k in good]) == PMD_ERR_ARG
    ctx.sync()
    assert bool(torch.isnan(Cd).all()) and bool(torch.isnan(Sd).all()) and bool(torch.isnan(rd).all())   # nothing launched
    assert bool((nd == -1).all())
    assert rc(ldc=0, C=null, lds=0, S=null) == 0         # a leading dimension of an output that is not asked for is not read
    ctx.sync()
    assert not bool(torch.isnan(rd).any())


# ---- deconvolve -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _five_traces():
    y = np.stack([R.planted(20 + k, T=600, g=(0.9, 0.95)[k % 2], sigma=SIGMA, rate=0.02)[0] for k in range(5)])
    y.setflags(write=False)
    return y


def _five_run(ctx):
    return OD.five_run(ctx, _five_traces(), 1)


def test_deconvolve_equals_the_reference(gpu_ctx):
    y = _five_traces()
    dc = _five_run(gpu_ctx)
    assert dc.calcium.shape == y.shape and dc.calcium.dtype == np.float32 and dc.spikes.dtype == np.float32
    assert dc.g.dtype == np.float32 and dc.noise.dtype == np.float64 and dc.lam.dtype == np.float32
    ref = R.deconvolve_ref(y, dc.g, dc.noise, rounds=3, points=4)
    _assert_result(dc, ref)
    _, sigma_ref = prep_ref.stats_ref(y.T)
    e = np.abs(dc.noise - sigma_ref) / sigma_ref
    print("noise against float64, relative:", e.max(), "g", dc.g, "lam", dc.lam, "evaluations", dc.evaluations)
    assert np.all(e <= SIGMA_RTOL)
    assert np.array_equal(dc.g, DX.estimate_decay(y, dc.noise).astype(np.float32))
    # three traces search all rounds; two leave by the first exit (their rss(0) is already above the target)
    assert np.all((dc.rss <= dc.noise ** 2 * 600) | (dc.lam == 0))
    assert np.all((dc.evaluations == 2 + 3 * 4 + 1) | (dc.evaluations == 3)) and np.sum(dc.evaluations == 15) >= 3


@pytest.mark.parametrize("launches", [1, 2, 20])
def test_deconvolve_bits_do_not_depend_on_the_workspace_cap(gpu_ctx, launches):
    """The largest round has 5 x 4 = 20 problems of 12 x 600 bytes each: caps that force one, two and twenty launches."""
    y = _five_traces()
    cap = 12 * 600 * (20 // launches)
    assert len(DX.launch_plan(20, 600, cap)) == launches
    dc = localmd_amd.deconvolve(y, search_rounds=3, search_points=4, max_workspace_bytes=cap, ctx=gpu_ctx)
    ref = _five_run(gpu_ctx)
    _assert_result(dc, {k: getattr(ref, k) for k in ("calcium", "spikes", "lam", "rss", "n_pools", "evaluations")})
    assert np.array_equal(dc.noise, ref.noise) and np.array_equal(dc.g, ref.g)


def test_deconvolve_fixed_penalty_and_single_trace(gpu_ctx):
    y = _five_traces()
    lam = np.float32([0.0, 0.5, 1.0, 2.0, 0.25])
    g = np.float32([0.9, 0.95, 0.9, 0.95, 0.5])
    s_min, b = np.float32([0, 0.2, 0, 0.1, 0]), np.float32([0, 0.1, -0.1, 0, 0])
    dc = localmd_amd.deconvolve(y, g=g, noise=SIGMA, lam=lam, s_min=s_min, baseline=b, ctx=gpu_ctx)
    for k in range(5):
        c, s, rss, npl = R.oasis_ar1(y[k], g[k], lam[k], s_min[k], b[k])
        assert np.array_equal(_bits(dc.calcium[k]), _bits(c)) and np.array_equal(_bits(dc.spikes[k]), _bits(s))
        assert dc.rss[k] == rss and dc.n_pools[k] == npl
    assert np.all(dc.evaluations == 1) and np.array_equal(dc.lam, lam) and np.all(dc.noise == SIGMA)
    assert np.array_equal(dc.baseline, b)
    # K = 1: the trace alone gets the bits it gets among the five
    ref = _five_run(gpu_ctx)
    one = localmd_amd.deconvolve(y[2:3], search_rounds=3, search_points=4, ctx=gpu_ctx)
    assert one.calcium.shape == (1, 600)
    assert np.array_equal(one.noise, ref.noise[2:3]) and np.array_equal(one.g, ref.g[2:3])
    _assert_result(one, {k: getattr(ref, k)[2:3] for k in ("calcium", "spikes", "lam", "rss", "n_pools", "evaluations")})


def test_planted_events_are_found_on_the_device(gpu_ctx):
    ys, truth = [], []
    for seed, rate in PLANTED:
        y, times, amps = R.planted(seed, rate=rate)
        ys.append(y), truth.append((times, amps))
    y = np.stack(ys)
    dc = localmd_amd.deconvolve(y, g=0.95, noise=SIGMA, ctx=gpu_ctx)
    for k, (times, amps) in enumerate(truth):
        hit, big, false_pos = R.planted_property(dc.spikes[k], times, amps, SIGMA)
        ratio = dc.rss[k] / (SIGMA ** 2 * y.shape[1])
        print("seed", PLANTED[k][0], "found", hit, "of", big, "false positives", false_pos, "rss / target", ratio)
        assert big >= 8 and hit >= 0.9 * big and false_pos == 0
        assert 0.999 <= ratio <= 1.0
    # the hand-over of the README: dF/F of the same traces on a baseline of 5 goes through with its own estimates
    dff = localmd_amd.trace_baseline(y + np.float32(5.0), window=600, ctx=gpu_ctx)
    out = localmd_amd.deconvolve(dff, ctx=gpu_ctx)
    assert out.spikes.shape == y.shape and np.all(np.isfinite(out.calcium)) and np.all(out.spikes >= 0)
    assert np.all((out.g >= 0) & (out.g < 1)) and np.all(out.noise > 0)


def test_device_memory_grows_by_the_resident_terms(gpu_ctx):
    import torch

    K, cap = 64, 12 * 4000 * 64          # one wave at T = 4000, a quarter of one at T = 16000; uncapped: 16 times that
    traces = _ar_traces(9, 16000, K).T
    peak = {}
    for T in (4000, 16000):
        y = traces[:, :T]
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(gpu_ctx.device)
        torch.cuda.reset_peak_memory_stats(gpu_ctx.device)
        localmd_amd.deconvolve(y, g=0.95, noise=SIGMA, search_rounds=1, search_points=4, max_workspace_bytes=cap,
                               ctx=gpu_ctx)
        peak[T] = torch.cuda.max_memory_allocated(gpu_ctx.device) - base
    slack = 1 << 20                        # the plan's allowance for the allocator's rounding of the small arrays
    resident = lambda T: 12 * K * T + 4 * K * (T + 1)     # noqa: E731
    print("peak", peak, "resident", resident(4000), resident(16000))
    assert peak[16000] - peak[4000] <= resident(16000) - resident(4000) + slack, peak
    plan = DX.deconvolve_device_bytes(K=K, T=16000, problems=4 * K, max_workspace_bytes=cap)
    assert resident(16000) <= peak[16000] <= plan, (peak, plan)
