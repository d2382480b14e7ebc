"""The percentile baseline on the GPU (pmd_sliding_quantile in csrc/baseline.hip; method="percentile" of
localmd_amd.baseline).  The kernel through the C ABI against the window sort of tests/baseline_quantile_ref.py: bit for
bit where the result is a number, NaN where it is NaN, over series lengths and windows around the kernel's slice, every
rank that matters, widths and leading dimensions on and off the 16-byte path, column ranges, data full of ties, ramps,
signed zeros, denormals, infinities and NaN runs; against pmd_sliding_extremum at the two end ranks; its bad arguments.
End to end rolling_baseline, dff_movie and trace_baseline with method="percentile" against the same reference applied
to the exported movie, invariance over batch sizes, sources, destinations and residency, how often the movie is read,
and the device memory that grows with the movie's length."""

import itertools

import numpy as np
import pytest

import localmd_amd
from localmd_amd import baseline as BL
from localmd_amd import decomposition as Dm
from localmd_amd._lib import PMDLibraryError, ptr
from localmd_amd.synthetic import make_movie
from tests import baseline_quantile_ref as Q
from tests import baseline_ref as R
from tests.test_gpu_baseline import POISON, _Counting, _dev, _extremum, _odd_ld, _padded
from tests.test_gpu_maps import _long_pmd

pytestmark = pytest.mark.gpu
Dm.QUIET = True
S = BL.QUANTILE_SLICE
NS = (1, 2, 5, 63, 64, 65, S - 1, S, S + 1, 2 * S + 1)
WIDTHS = (1, 3, 4, 5, 255, 256, 257, 260)
NAN = np.float32(np.nan)


def _ranks(h, q=0.08):
    return sorted({0, 1 % (2 * h + 1), h, max(0, 2 * h - 1), 2 * h, Q.rank_of(h, q)})


def _quantile(ctx, xd, ldx, n, N, h, rank, ldo, *, ranges=None, c_in=0):
    """pmd_sliding_quantile on the columns c_in .. c_in + N of the device matrix, one call per column range, into a
    poisoned (n, ldo) matrix at the same columns; everything else of it must keep the poison."""
    out = _dev(ctx, np.full((n, ldo), POISON, np.float32))
    for c0, c1 in ([(0, N)] if ranges is None else ranges):
        assert ctx.lib.pmd_sliding_quantile_work_floats(n, c1 - c0, h) == 0
        ctx.call("pmd_sliding_quantile", BL._offset(xd, c_in + c0), ldx, n, c1 - c0, h, rank, BL._offset(out, c_in + c0),
                 ldo, None, 0)
    ctx.sync()
    out = out.cpu().numpy()
    assert np.all(out[:, :c_in] == POISON) and np.all(out[:, c_in + N:] == POISON)
    return out[:, c_in:c_in + N]


def _layout(x, which):
    """(host matrix holding x, ld, first column): 0 a padded 16-byte aligned leading dimension, 1 an odd one, 2 the
    columns 5 .. 5 + N of a wider matrix, 3 the columns 4 .. 4 + N of a wider aligned one; paddings are NaN."""
    n, N = x.shape
    if which == 0:
        return _padded(x, (N + 7) // 4 * 4, NAN), (N + 7) // 4 * 4, 0
    if which == 1:
        return _padded(x, _odd_ld(N), NAN), _odd_ld(N), 0
    c_in, ld = (5, N + 9) if which == 2 else (4, (N + 15) // 4 * 4)
    wide = np.full((n, ld), NAN, np.float32)
    wide[:, c_in:c_in + N] = x
    return wide, ld, c_in


# ---- pmd_sliding_quantile ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_sliding_quantile_equals_the_window_sort(gpu_ctx, n):
    rng = np.random.default_rng(100 + n)
    for i, h in enumerate(sorted({0, 1, 2, 7, 31, 32, n - 1, n, 3 * n} - {-1})):
        W = 2 * h + 1
        N = WIDTHS[(i + n) % len(WIDTHS)]
        if n * W * N > 2e7:                       # the reference sorts n W N keys: long windows get the narrow widths
            N = WIDTHS[(i + n) % 4]
        x = Q.series(rng, n, N, h, shift=i + n)
        host, ld, c_in = _layout(x, (i + n) % 4)
        xd = _dev(gpu_ctx, host)
        want = Q.sliding_ranks(x, h, _ranks(h))
        for k, ref in want.items():
            got = _quantile(gpu_ctx, xd, ld, n, N, h, k, ld + (k % 2), c_in=c_in)
            assert R.same_bits(got, ref), (n, h, N, ld, c_in, k)


@pytest.mark.parametrize("N", WIDTHS)
def test_every_width_in_every_layout(gpu_ctx, N):
    rng = np.random.default_rng(200 + N)
    for n, h in ((S + 1, 7), (65, 32)):
        x = Q.series(rng, n, N, h, shift=N)
        want = Q.sliding_ranks(x, h, _ranks(h))
        for which in range(4):
            host, ld, c_in = _layout(x, which)
            xd = _dev(gpu_ctx, host)
            for k, ref in want.items():
                got = _quantile(gpu_ctx, xd, ld, n, N, h, k, ld, c_in=c_in)
                assert R.same_bits(got, ref), (n, h, N, which, k)


def test_every_kind_of_series_around_the_slice(gpu_ctx):
    """All twelve kinds of column twice over, with NaN runs shorter than, equal to and longer than the window."""
    rng = np.random.default_rng(300)
    N = 2 * len(Q.SERIES_KINDS)
    for n, h in ((S + 9, 3), (2 * S + 1, 31), (S, 2 * S)):
        x = Q.series(rng, n, N, h)
        assert np.isnan(x[:, 8:12]).any(axis=0).all() and np.isnan(x[:, 11]).all() and not np.isnan(x[:, :8]).any()
        xd = _dev(gpu_ctx, x)
        want = Q.sliding_ranks(x, h, _ranks(h))
        for k, ref in want.items():
            got = _quantile(gpu_ctx, xd, N, n, N, h, k, N)
            assert R.same_bits(got, ref), (n, h, k)
            assert np.all(np.isnan(got[:, 11])) and np.all(got[:, 2] == np.float32(2.5))
            nan = np.isnan(got)
            assert np.all(got.view(np.uint32)[nan] == 0x7FFFFFFF)          # key_floats of the NaN key
    # the bits of a zero are those of the member at the rank, not of an equal one
    z = np.array([[0.0, -0.0], [-0.0, 0.0], [0.0, 0.0], [-0.0, -0.0], [0.0, -0.0]], np.float32)
    zd = _dev(gpu_ctx, z)
    for k in range(3):
        got = _quantile(gpu_ctx, zd, 2, 5, 2, 1, k, 2)
        assert got.tobytes() == Q.sliding_rank(z, 1, k).tobytes(), k
    assert np.signbit(_quantile(gpu_ctx, zd, 2, 5, 2, 1, 1, 2)).tolist() == [[False, True], [False, False], [True, False],
                                                                            [False, True], [False, True]]


def test_a_window_of_two_to_the_31_members(gpu_ctx):
    """half = 2^30 - 1: every count of a window fits 32 bits, and the work does not grow with the replicated copies."""
    rng = np.random.default_rng(400)
    n, h = 5, 2 ** 30 - 1
    x = Q.series(rng, n, 12, 1)
    xd = _dev(gpu_ctx, x)
    for k in (0, 1, h - 2, h, h + 2, 2 * h - 1, 2 * h):
        got = _quantile(gpu_ctx, xd, 12, n, 12, h, k, 12)
        assert R.same_bits(got, Q.weighted_rank(x, h, k)), k


def test_column_bits_do_not_depend_on_the_neighbours_or_the_split(gpu_ctx):
    rng = np.random.default_rng(500)
    n, h = S + 5, 9
    k = Q.rank_of(h, 0.08)
    # every split of six columns into ranges, and every column alone
    x = Q.series(rng, n, 6, h, shift=3)
    for ld in (6, 8, 9):
        xd = _dev(gpu_ctx, _padded(x, ld, NAN))
        one = _quantile(gpu_ctx, xd, ld, n, 6, h, k, ld)
        assert R.same_bits(one, Q.sliding_rank(x, h, k))
        for cuts in itertools.chain.from_iterable(itertools.combinations(range(1, 6), r) for r in range(1, 6)):
            edges = (0,) + cuts + (6,)
            got = _quantile(gpu_ctx, xd, ld, n, 6, h, k, ld, ranges=list(zip(edges[:-1], edges[1:])))
            assert got.tobytes() == one.tobytes(), (ld, cuts)
    # a wide matrix: ranges of 64 and of 7 columns, one column and the rest, and columns alone in a matrix of their own
    N = 300
    x = Q.series(rng, n, N, h)
    for ld in (N, N + 1):
        xd = _dev(gpu_ctx, _padded(x, ld, NAN))
        one = _quantile(gpu_ctx, xd, ld, n, N, h, k, ld)
        assert R.same_bits(one, Q.sliding_rank(x, h, k))
        for step in (64, 7):
            ranges = [(c0, min(N, c0 + step)) for c0 in range(0, N, step)]
            assert _quantile(gpu_ctx, xd, ld, n, N, h, k, ld, ranges=ranges).tobytes() == one.tobytes(), (ld, step)
        assert _quantile(gpu_ctx, xd, ld, n, N, h, k, ld, ranges=[(0, 1), (1, N)]).tobytes() == one.tobytes()
    for c in (0, 7, 130, 299):
        alone = _quantile(gpu_ctx, _dev(gpu_ctx, x[:, c:c + 1]), 1, n, 1, h, k, 1)
        assert alone.tobytes() == one[:, c:c + 1].tobytes(), c


def test_end_ranks_equal_the_sliding_extrema(gpu_ctx):
    rng = np.random.default_rng(600)
    for n, N, h in ((S + 3, 70, 5), (40, 9, 60), (2 * S + 1, 257, 32)):
        x = rng.integers(-5, 6, (n, N)).astype(np.float32) + rng.standard_normal((n, N)).astype(np.float32)
        xd = _dev(gpu_ctx, x)
        for is_max in (False, True):
            ext = _extremum(gpu_ctx, xd, N, n, N, h, is_max, N)
            got = _quantile(gpu_ctx, xd, N, n, N, h, 2 * h if is_max else 0, N)
            assert np.array_equal(got, ext), (n, N, h, is_max)


def test_sliding_quantile_rejects_bad_arguments(gpu_ctx):
    import torch

    n, N = 10, 35
    f32 = dict(dtype=torch.float32, device=gpu_ctx.device)
    x = torch.zeros((n, 40), **f32)
    out = torch.full((n, 40), 5.0, **f32)
    work = torch.zeros(16, **f32)
    names = ["X", "ldx", "n", "N", "half", "rank", "out", "ldo", "work", "work_floats"]
    good = [ptr(x), 40, n, N, 2, 1, ptr(out), 40, None, 0]

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        with pytest.raises(PMDLibraryError, match=r"failed \(-2\)"):      # PMD_ERR_ARG
            gpu_ctx.call("pmd_sliding_quantile", *a)

    big = 65535 * 256 + 1
    for kw in (dict(n=0), dict(n=-1), dict(n=2 ** 31), dict(N=0), dict(N=-3), dict(N=big, ldx=big, ldo=big), dict(ldx=N - 1),
               dict(ldo=N - 1), dict(half=-1), dict(half=2 ** 30, rank=0), dict(rank=-1), dict(rank=5), dict(half=0, rank=1),
               dict(X=None), dict(out=None), dict(out=ptr(x)), dict(out=BL._offset(x, 40 * 3)),
               dict(out=BL._offset(x, 40 * 9 + 34)), dict(work_floats=-1), dict(work=ptr(work), work_floats=-1)):
        bad(**kw)
    gpu_ctx.sync()
    assert bool((out == 5.0).all())
    gpu_ctx.call("pmd_sliding_quantile", *good)
    gpu_ctx.sync()
    assert bool((out[:, :N] == 0).all()) and bool((out[:, N:] == 5.0).all())
    # a workspace larger than asked for is fine, and out may start right behind X's last element
    y = torch.zeros(n * 40 + n * 40, **f32)
    gpu_ctx.call("pmd_sliding_quantile", ptr(y), 40, n, N, 2, 4, BL._offset(y, 40 * 9 + 35), 40, ptr(work), 16)
    gpu_ctx.sync()


# ---- end to end ----------------------------------------------------------------------------------------------------
T, D1, D2 = 2100, 40, 40
D = D1 * D2
WINDOW, BIN, QQ = 300, 16, 0.08


@pytest.fixture(scope="module")
def case(gpu_ctx):
    """An integer-valued bleaching movie (exact in uint16) decomposed once, the fp32 denoised movie export_movie writes,
    and the reference dF/F of both kinds."""
    t = np.arange(T, dtype=np.float64)[:, None, None]
    mov = np.rint(8.0 * make_movie(T, D1, D2, seed=4) * (0.6 + 0.4 * np.exp(-t / 800.0))).astype(np.float32)
    np.random.seed(0)
    pmd = localmd_amd.localmd_decomposition(mov, (20, 20), 1000, max_components=4, background_rank=1, seed=3,
                                            sim_iters=5, order="F", ctx=gpu_ctx)
    den = np.empty((T, D1, D2), np.float32)
    localmd_amd.export_movie(pmd, den, panels="denoised", dtype="float32", ctx=gpu_ctx)
    h = R.half_of(WINDOW, BIN)
    ref = {kind: Q.dff(y.reshape(T, D), BIN, h, QQ, "dff") for kind, y in (("denoised", den), ("raw", mov))}
    return {"mov": mov, "pmd": pmd, "denoised": den.reshape(T, D), "raw": mov.reshape(T, D), "ref": ref, "h": h}


@pytest.mark.parametrize("kind", ["denoised", "raw"])
def test_rolling_baseline_percentile_knots_bit_for_bit(gpu_ctx, case, kind):
    y, pmd = case[kind], case["pmd"]
    movie = case["mov"] if kind == "raw" else None
    for b, window, q in ((BIN, WINDOW, None), (BIN, WINDOW, 0.5), (1, 21, 0.08), (1, 21, 1.0)):
        bl = localmd_amd.rolling_baseline(pmd, movie, kind=kind, window=window, temporal_bin=b, method="percentile", q=q,
                                          ctx=gpu_ctx)
        h = R.half_of(window, b)
        want = Q.filtered_percentile(R.movie_knots(y, b), h, 0.08 if q is None else q)
        assert bl.knots.shape == (-(-T // b), D1, D2) and bl.knots.dtype == np.float32
        assert bl.knots.reshape(-1, D).tobytes() == want.tobytes(), (b, q)
        assert (bl.temporal_bin, bl.window_frames, bl.method, bl.kind, bl.n_frames) == (b, (2 * h + 1) * b, "percentile", kind, T)
        assert bl.q == (0.08 if q is None else q) and "percentile q=" in repr(bl)
    bl = pmd.baseline(movie, kind=kind, window=WINDOW, method="percentile", ctx=gpu_ctx)
    assert bl.knots.reshape(-1, D).tobytes() == case["ref"][kind][0].tobytes()
    # a percentile lies between the extrema of the same window
    lo = localmd_amd.rolling_baseline(pmd, movie, kind=kind, window=WINDOW, method="minimum", ctx=gpu_ctx)
    assert np.all(lo.knots <= bl.knots) and lo.q is None


@pytest.mark.parametrize("kind", ["denoised", "raw"])
def test_dff_movie_percentile_every_output_bit_for_bit(gpu_ctx, case, kind):
    y, pmd = case[kind], case["pmd"]
    movie = case["mov"] if kind == "raw" else None
    K = case["ref"][kind][0]
    F0 = R.baseline_frames(K, T, BIN, 0, T)
    bl = localmd_amd.rolling_baseline(pmd, movie, kind=kind, window=WINDOW, method="percentile", ctx=gpu_ctx)
    for output in BL.OUTPUTS:
        out = np.full((T, D1, D2), POISON, np.float32)
        got = localmd_amd.dff_movie(pmd, out, movie, kind=kind, output=output, window=WINDOW, method="percentile", q=QQ,
                                    ctx=gpu_ctx)
        assert got is out
        assert out.reshape(T, D).tobytes() == R.outputs(y, F0, output).tobytes(), output
        two = np.empty((T, D1, D2), np.float32)
        pmd.dff(two, movie, kind=kind, output=output, baseline=bl, ctx=gpu_ctx)
        assert two.tobytes() == out.tobytes(), output
    assert case["ref"][kind][1].tobytes() == R.outputs(y, F0, "dff").tobytes()


def test_trace_baseline_percentile_equals_the_pixels_of_dff_movie(gpu_ctx, case):
    px = np.array([0, 1, 39, 40, 1000, D - 1])
    for kind in ("denoised", "raw"):
        y = case[kind]
        F0 = R.baseline_frames(case["ref"][kind][0], T, BIN, 0, T)
        for output in BL.OUTPUTS:
            got = localmd_amd.trace_baseline(y[:, px].T, window=WINDOW, method="percentile", output=output, ctx=gpu_ctx)
            assert got.shape == (len(px), T) and got.dtype == np.float32
            assert got.tobytes() == np.ascontiguousarray(R.outputs(y, F0, output)[:, px].T).tobytes(), (kind, output)
    # temporal_bin = 1: the percentile filter on the frames themselves
    x = case["raw"][:700, :3]
    got = localmd_amd.trace_baseline(x.T, window=101, temporal_bin=1, method="percentile", q=0.2, output="baseline",
                                     ctx=gpu_ctx)
    assert got.tobytes() == np.ascontiguousarray(Q.filtered_percentile(x, 50, 0.2).T).tobytes()


def test_invariance_over_batches_sources_destinations_and_residency(gpu_ctx, case, tmp_path):
    import torch

    pmd, mov = case["pmd"], case["mov"]
    want = {kind: case["ref"][kind][1].tobytes() for kind in ("denoised", "raw")}
    knots = {kind: case["ref"][kind][0].tobytes() for kind in ("denoised", "raw")}
    kw = dict(window=WINDOW, method="percentile", ctx=gpu_ctx)

    def run(kind, movie, **more):
        out = np.empty((T, D1, D2), np.float32)
        localmd_amd.dff_movie(pmd, out, movie, kind=kind, **more, **kw)
        return out.tobytes()

    for fbs in (1024, 2048, 10000):
        assert run("denoised", None, frame_batch_size=fbs) == want["denoised"], fbs
        assert run("raw", mov, frame_batch_size=fbs) == want["raw"], fbs
        bl = localmd_amd.rolling_baseline(pmd, mov, kind="raw", frame_batch_size=fbs, **kw)
        assert bl.knots.tobytes() == knots["raw"], fbs
    u16 = mov.astype(np.uint16)
    sources = {"numpy_u16": u16, "cpu_tensor": torch.from_numpy(mov), "device_tensor": torch.from_numpy(mov).to(gpu_ctx.device)}
    for name, src in sources.items():
        assert run("raw", src, frame_batch_size=2048) == want["raw"], name
    for kind, movie in (("denoised", None), ("raw", u16)):
        npy = localmd_amd.dff_movie(pmd, str(tmp_path / (kind + ".npy")), movie, kind=kind, frame_batch_size=1024, **kw)
        assert np.load(npy).tobytes() == want[kind], kind
        dev = torch.full((T, D1, D2), float(POISON), dtype=torch.float32, device=gpu_ctx.device)
        assert localmd_amd.dff_movie(pmd, dev, movie, kind=kind, **kw) is dev
        assert dev.cpu().numpy().tobytes() == want[kind], kind
    pmd.to_device(ctx=gpu_ctx)
    try:
        out = np.empty((T, D1, D2), np.float32)
        pmd.dff(out, window=WINDOW, method="percentile")
        assert out.tobytes() == want["denoised"]
        assert pmd.baseline(u16, kind="raw", window=WINDOW, method="percentile").knots.tobytes() == knots["raw"]
    finally:
        pmd.to_host()


def test_movie_reads(gpu_ctx, case):
    """Raw: every frame once for the knots, twice for dff_movie, once with a given percentile baseline."""
    pmd = case["pmd"]
    u16 = case["mov"].astype(np.uint16)
    out = np.empty((T, D1, D2), np.float32)
    kw = dict(kind="raw", frame_batch_size=1024, ctx=gpu_ctx)
    src = _Counting(u16)
    bl = localmd_amd.rolling_baseline(pmd, src, window=WINDOW, method="percentile", **kw)
    assert np.all(src.count == 1), np.unique(src.count)
    assert bl.knots.tobytes() == case["ref"]["raw"][0].tobytes()
    src = _Counting(u16)
    localmd_amd.dff_movie(pmd, out, src, window=WINDOW, method="percentile", **kw)
    assert np.all(src.count == 2), np.unique(src.count)
    assert out.reshape(T, D).tobytes() == case["ref"]["raw"][1].tobytes()
    src = _Counting(u16)
    localmd_amd.dff_movie(pmd, out, src, baseline=bl, **kw)
    assert np.all(src.count == 1), np.unique(src.count)
    assert out.reshape(T, D).tobytes() == case["ref"]["raw"][1].tobytes()


def test_device_memory_grows_by_the_knot_terms_only(gpu_ctx):
    import torch

    d1 = d2 = 64
    h = BL.half_window(WINDOW, 16)
    peaks = {}
    for n in (4096, 8192):
        pmd = _long_pmd(n, d1, d2)
        gpu_ctx.release_workspace()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = np.empty((n, d1, d2), np.float32)
        localmd_amd.dff_movie(pmd, out, kind="denoised", window=WINDOW, method="percentile", frame_batch_size=4096,
                              ctx=gpu_ctx)
        peaks[n] = torch.cuda.max_memory_allocated() - base
        assert np.all(np.isfinite(out))
    grow = BL.knot_bytes(8192, d1 * d2, 16, "percentile", h) - BL.knot_bytes(4096, d1 * d2, 16, "percentile", h)
    print("peak device bytes", peaks, "knot terms grow by", grow)
    assert grow == 2 * 4 * 256 * d1 * d2                      # the knots and the filter's output: no workspace
    assert peaks[8192] - peaks[4096] <= grow, (peaks, grow)
