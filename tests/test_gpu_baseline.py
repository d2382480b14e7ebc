"""Rolling-baseline dF/F on the GPU (localmd_amd.baseline, csrc/baseline.hip).  pmd_bin_means, pmd_sliding_extremum and
pmd_baseline_apply through the C ABI against the NumPy emulations of tests/baseline_ref.py (bit for bit; the sliding
extrema by value, as -0 and +0 tie), their bad arguments; end to end rolling_baseline, dff_movie and trace_baseline
against the same emulations applied to the exported movie, invariance over batch sizes, sources, destinations and
residency, how often the movie is read, the device memory that grows with the movie's length, and a failed export.

"Bit for bit" leaves one thing open: the sign and payload of a NaN that arithmetic produced (inf - inf) differ between
processors, so any NaN matches any NaN (baseline_ref.same_bits)."""

import numpy as np
import pytest

import localmd_amd
from localmd_amd import baseline as BL
from localmd_amd import decomposition as Dm
from localmd_amd._lib import PMDLibraryError, ptr
from localmd_amd.dataset import TiffArray, lazy_data_loader
from localmd_amd.synthetic import make_movie
from tests import baseline_ref as R
from tests.test_gpu_maps import _long_pmd

pytestmark = pytest.mark.gpu
Dm.QUIET = True
_ELEM = {"float32": 0, "uint16": 1, "int16": 2}
_FILL = {"float32": np.nan, "uint16": 65535, "int16": -32768}      # paddings of an input: they would show up
POISON = np.float32(-7777.0)                                        # paddings of an output: they must stay


def _dev(ctx, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _padded(a, ld, fill):
    out = np.full((a.shape[0], ld), fill, dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out


def _odd_ld(N):
    """A leading dimension above N that is odd: no row after the first is 16-byte aligned."""
    return N + 3 if (N + 3) % 2 else N + 4


# ---- pmd_bin_means -------------------------------------------------------------------------------------------------
def _values(rng, src, shape):
    if src == "float32":
        return (900.0 + 8.0 * rng.standard_normal(shape)).astype(np.float32)
    if src == "uint16":
        return rng.integers(0, 65536, shape).astype(np.uint16)
    return rng.integers(-32768, 32768, shape).astype(np.int16)


def _bin_means(ctx, yd, src, ldy, n, N, f0, bin, ldk):
    """One call on the first n rows of the device batch; returns (the knot rows of the call, everything else)."""
    rows = (f0 + n + bin - 1) // bin + 1
    K = _dev(ctx, np.full((rows, ldk), POISON, np.float32))
    ctx.call("pmd_bin_means", ptr(yd), _ELEM[src], ldy, n, N, f0, bin, ptr(K), ldk)
    ctx.sync()
    K = K.cpu().numpy()
    r0, r1 = f0 // bin, (f0 + n + bin - 1) // bin
    rest = np.concatenate([K[:r0].reshape(-1), K[r1:].reshape(-1), K[r0:r1, N:].reshape(-1)])
    return K[r0:r1, :N], rest


@pytest.mark.parametrize("src", list(_ELEM))
def test_bin_means_bit_for_bit(gpu_ctx, src):
    rng = np.random.default_rng(1)
    for N in (1, 63, 64, 65, 257):
        Y = _values(rng, src, (1024, N))
        for ldy, ldk in ((_odd_ld(N), _odd_ld(N) + 2), ((N + 15) // 8 * 8, (N + 7) // 4 * 4)):
            yd = _dev(gpu_ctx, _padded(Y, ldy, _FILL[src]))
            for n in (1, 255, 256, 257, 1024):
                for bin in (1, 2, 32, 256):
                    want = R.bin_chain(Y[:n], bin)
                    for f0 in (0, 1024):
                        got, rest = _bin_means(gpu_ctx, yd, src, ldy, n, N, f0, bin, ldk)
                        key = (N, ldy, ldk, n, bin, f0)
                        assert got.tobytes() == want.tobytes(), key
                        assert np.all(rest == POISON), key


def test_bin_means_nan_and_inf(gpu_ctx):
    rng = np.random.default_rng(2)
    n, N = 1000, 65
    Y = _values(rng, "float32", (n, N))
    Y[3, 0] = np.nan
    Y[40:44, 1] = np.inf
    Y[50, 2], Y[51, 2] = np.inf, -np.inf                                # inf - inf inside a bin
    Y[999, 3] = -np.inf                                                # in the short last bin
    Y[64:96, 4] = np.nan
    for ldy in (N, 72):
        yd = _dev(gpu_ctx, _padded(Y, ldy, np.nan))
        for bin in (1, 2, 32, 256):
            got, _ = _bin_means(gpu_ctx, yd, "float32", ldy, n, N, 2048, bin, N)
            want = R.bin_chain(Y, bin)
            assert R.same_bits(got, want), (ldy, bin)
            assert np.isnan(got[3 // bin, 0]) and np.isnan(got[50 // bin, 2]) == (bin > 1)
            assert got[999 // bin, 3] == -np.inf and np.all(np.isfinite(got[:, 5:]))


def test_bin_means_rejects_bad_arguments(gpu_ctx):
    import torch

    N = 35
    y = torch.zeros((8, 40), dtype=torch.float32, device=gpu_ctx.device)
    K = torch.full((8, 40), 5.0, dtype=torch.float32, device=gpu_ctx.device)
    names = ["Y", "elem", "ldy", "n", "N", "f0", "bin", "K", "ldk"]
    good = [ptr(y), 0, 40, 4, N, 0, 2, ptr(K), 40]

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        with pytest.raises(PMDLibraryError, match=r"failed \(-2\)"):      # PMD_ERR_ARG
            gpu_ctx.call("pmd_bin_means", *a)

    for kw in (dict(n=0), dict(n=-1), dict(n=1025), dict(bin=0), dict(bin=3), dict(bin=512), dict(bin=-4),
               dict(bin=8, f0=4), dict(f0=-2), dict(f0=2 ** 31 - 4), dict(elem=3), dict(elem=-1), dict(ldy=N - 1),
               dict(ldk=N - 1), dict(N=0), dict(Y=None), dict(K=None)):
        bad(**kw)
    gpu_ctx.sync()
    assert bool((K == 5.0).all())
    gpu_ctx.call("pmd_bin_means", *good)
    gpu_ctx.sync()
    assert bool((K[:2, :N] == 0).all()) and bool((K[2:] == 5.0).all()) and bool((K[:, N:] == 5.0).all())


# ---- pmd_sliding_extremum ------------------------------------------------------------------------------------------
def _series(rng, n, N, h, shift):
    """(n, N) float32 whose columns cycle through: integers full of ties, the same with +-inf, with a NaN run shorter
    than the window, with a NaN run longer than the window, all NaN; ``shift`` moves the cycle."""
    W = 2 * h + 1
    x = rng.integers(-5, 6, (n, N)).astype(np.float32)
    x[x == 0] = np.where(rng.random(int((x == 0).sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    for c in range(N):
        kind = (c + shift) % 5
        at = int(rng.integers(0, n))
        if kind == 1:
            x[rng.random(n) < 0.1, c] = np.inf
            x[rng.random(n) < 0.1, c] = -np.inf
        elif kind == 2:
            x[at:at + h, c] = np.nan
        elif kind == 3:
            x[at:at + W + 2, c] = np.nan
        elif kind == 4:
            x[:, c] = np.nan
    return x


def _extremum(ctx, xd, ldx, n, N, h, is_max, ldo, *, ranges=None, work_floats=None):
    import torch

    out = _dev(ctx, np.full((n, ldo), POISON, np.float32))
    ranges = [(0, N)] if ranges is None else ranges
    need = max(n * (-(-(c1 - c0) // 4) * 4) for c0, c1 in ranges)
    assert need == max(ctx.lib.pmd_sliding_extremum_work_floats(n, c1 - c0) for c0, c1 in ranges)
    work_floats = need if work_floats is None else work_floats
    work = torch.full((work_floats + 8,), float(POISON), dtype=torch.float32, device=ctx.device)
    for c0, c1 in ranges:
        ctx.call("pmd_sliding_extremum", BL._offset(xd, c0), ldx, n, c1 - c0, h, int(is_max), BL._offset(out, c0), ldo,
                 ptr(work), work_floats)
    ctx.sync()
    assert bool((work[work_floats:] == float(POISON)).all())
    out = out.cpu().numpy()
    assert np.all(out[:, N:] == POISON)
    return out[:, :N]


@pytest.mark.parametrize("h", [0, 1, 2, 7, 100])
def test_sliding_extremum_equals_the_emulation(gpu_ctx, h):
    rng = np.random.default_rng(3 + h)
    W = 2 * h + 1
    for n in sorted({1, 2, W - 1, W, W + 1, 2 * W, 3 * W + 5, 1000} - {0}):
        for i, N in enumerate((1, 64, 65, 300)):
            x = _series(rng, n, N, h, shift=n + i)
            ldx, ldo = (N + 3, N + 1) if i % 2 else ((N + 7) // 4 * 4, (N + 11) // 4 * 4)
            xd = _dev(gpu_ctx, _padded(x, ldx, np.float32(np.nan)))
            for is_max in (False, True):
                got = _extremum(gpu_ctx, xd, ldx, n, N, h, is_max, ldo)
                assert np.array_equal(got, R.sliding(x, h, is_max), equal_nan=True), (h, n, N, is_max)


def test_sliding_extremum_window_beyond_the_series_and_column_ranges(gpu_ctx):
    rng = np.random.default_rng(9)
    n, N = 7, 65
    x = _series(rng, n, N, 3, shift=0)
    xd = _dev(gpu_ctx, x)
    for h in (6, 7, 1000, 2 ** 40):                     # half >= n - 1: every window is the whole series
        for is_max in (False, True):
            got = _extremum(gpu_ctx, xd, N, n, N, h, is_max, N)
            want = np.broadcast_to((np.fmax if is_max else np.fmin).reduce(x, axis=0), (n, N))
            assert np.array_equal(got, want, equal_nan=True), (h, is_max)
    # ranges of 64 columns with the workspace of one range equal one call over all columns
    n, N, h = 500, 300, 7
    x = _series(rng, n, N, h, shift=1)
    for ld in (N, N + 1):
        xd = _dev(gpu_ctx, _padded(x, ld, np.float32(np.nan)))
        ranges = [(c0, min(N, c0 + 64)) for c0 in range(0, N, 64)]
        for is_max in (False, True):
            one = _extremum(gpu_ctx, xd, ld, n, N, h, is_max, ld)
            walked = _extremum(gpu_ctx, xd, ld, n, N, h, is_max, ld, ranges=ranges, work_floats=n * 64)
            assert np.array_equal(one, R.sliding(x, h, is_max), equal_nan=True)
            assert np.array_equal(one, walked, equal_nan=True) and np.array_equal(np.signbit(one), np.signbit(walked))


def test_sliding_extremum_rejects_bad_arguments(gpu_ctx):
    import torch

    n, N = 10, 35
    f32 = dict(dtype=torch.float32, device=gpu_ctx.device)
    x = torch.zeros((n, 40), **f32)
    out = torch.full((n, 40), 5.0, **f32)
    work = torch.zeros(n * 36, **f32)
    names = ["X", "ldx", "n", "N", "half", "is_max", "out", "ldo", "work", "work_floats"]
    good = [ptr(x), 40, n, N, 2, 0, ptr(out), 40, ptr(work), n * 36]

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        with pytest.raises(PMDLibraryError, match=r"failed \(-2\)"):
            gpu_ctx.call("pmd_sliding_extremum", *a)

    for kw in (dict(n=0), dict(n=-1), dict(N=0), dict(ldx=N - 1), dict(ldo=N - 1), dict(half=-1), dict(is_max=2),
               dict(is_max=-1), dict(X=None), dict(out=None), dict(work=None), dict(work_floats=n * 36 - 1),
               dict(work_floats=0), dict(out=ptr(x)), dict(out=BL._offset(x, 40 * 3)), dict(out=BL._offset(x, 40 * 9 + 34))):
        bad(**kw)
    gpu_ctx.sync()
    assert bool((out == 5.0).all())
    gpu_ctx.call("pmd_sliding_extremum", *good)
    gpu_ctx.sync()
    assert bool((out[:, :N] == 0).all()) and bool((out[:, N:] == 5.0).all())
    # out may start right behind X's last element
    y = torch.zeros(n * 40 + n * 40, **f32)
    gpu_ctx.call("pmd_sliding_extremum", ptr(y), 40, n, N, 2, 1, BL._offset(y, 40 * 9 + 35), 40, ptr(work), n * 36)
    gpu_ctx.sync()


# ---- pmd_baseline_apply --------------------------------------------------------------------------------------------
T_APPLY = 2248          # two full blocks and 200 frames; with bins of 32 the last bin has 8 frames


def _apply(ctx, xd, src, ldx, n, N, f0, T, bin, kd, ldk, mode, min_baseline, ldo):
    out = _dev(ctx, np.full((n, ldo), POISON, np.float32))
    ctx.call("pmd_baseline_apply", ptr(xd), _ELEM[src], ldx, n, N, f0, T, bin, ptr(kd), ldk, mode, float(min_baseline),
             ptr(out), ldo)
    ctx.sync()
    out = out.cpu().numpy()
    assert np.all(out[:, N:] == POISON)
    return out[:, :N]


@pytest.mark.parametrize("bin", [1, 32, 256])
@pytest.mark.parametrize("src", ["float32", "uint16"])
def test_baseline_apply_bit_for_bit(gpu_ctx, src, bin):
    rng = np.random.default_rng(4)
    T = T_APPLY
    assert T == 2 * 1024 + 200 and T % 32 == 8
    n_bins = -(-T // bin)
    for N, ldx, ldk, ldo in ((521, _odd_ld(521), 523, 525), (520, 528, 520, 524)):
        X = _values(rng, src, (T, N)) if src == "float32" else rng.integers(0, 2000, (T, N)).astype(np.uint16)
        K = (900.0 + 300.0 * rng.standard_normal((n_bins, N))).astype(np.float32)
        K[:, 3] = -np.abs(K[:, 3])                                           # a baseline that is not positive
        K[n_bins // 2:, 4] = 0.0
        K[:: max(1, n_bins // 5), 5] = np.nan                          # NaN knots
        K[n_bins // 3, 6] = np.inf
        kd = _dev(gpu_ctx, _padded(K, ldk, np.float32(np.nan)))
        for min_baseline in (0.0, 700.0):
            F0 = R.baseline_frames(K, T, bin, 0, T)
            for f0 in (0, 1024, 2048):
                n = min(1024, T - f0)
                xd = _dev(gpu_ctx, _padded(X[f0:f0 + n], ldx, _FILL[src]))
                for mode, output in enumerate(BL.OUTPUTS):
                    if mode < 2 and min_baseline:
                        continue
                    got = _apply(gpu_ctx, xd, src, ldx, n, N, f0, T, bin, kd, ldk, mode, min_baseline, ldo)
                    want = R.outputs(X[f0:f0 + n], F0[f0:f0 + n], output, min_baseline)
                    key = (N, min_baseline, f0, output)
                    assert R.same_bits(got, want), key
                    if mode == 2:       # where F0 > min_baseline does not hold, a NaN F0 included: 0
                        off = ~(F0[f0:f0 + n] > np.float32(min_baseline))
                        assert off[:, 3].all() and off[:, 5].any() and np.all(got[off] == 0), key
                    if mode == 0:       # X is not read: NULL, and any element type
                        null = _apply(gpu_ctx, None, "int16", 0, n, N, f0, T, bin, kd, ldk, 0, 0.0, ldo)
                        assert R.same_bits(null, want), key


def test_baseline_apply_rejects_bad_arguments(gpu_ctx):
    import torch

    N, T = 35, 100
    f32 = dict(dtype=torch.float32, device=gpu_ctx.device)
    x = torch.ones((8, 40), **f32)
    K = torch.ones((25, 40), **f32)
    out = torch.full((8, 40), 5.0, **f32)
    names = ["X", "elem", "ldx", "n", "N", "f0", "T", "bin", "K", "ldk", "mode", "min_baseline", "out", "ldo"]
    good = [ptr(x), 0, 40, 8, N, 16, T, 4, ptr(K), 40, 2, 0.0, ptr(out), 40]

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        with pytest.raises(PMDLibraryError, match=r"failed \(-2\)"):
            gpu_ctx.call("pmd_baseline_apply", *a)

    for kw in (dict(n=0), dict(n=1025), dict(N=0), dict(ldx=N - 1), dict(ldk=N - 1), dict(ldo=N - 1), dict(f0=-1),
               dict(f0=T - 7), dict(T=0), dict(T=2 ** 23), dict(bin=0), dict(bin=3), dict(bin=512), dict(mode=3),
               dict(mode=-1), dict(elem=5), dict(X=None), dict(X=None, mode=1), dict(K=None), dict(out=None)):
        bad(**kw)
    gpu_ctx.sync()
    assert bool((out == 5.0).all())
    gpu_ctx.call("pmd_baseline_apply", *good)
    gpu_ctx.sync()
    assert bool((out[:, :N] == 0).all()) and bool((out[:, N:] == 5.0).all())


# ---- end to end ----------------------------------------------------------------------------------------------------
T, D1, D2 = 2248, 40, 48
D = D1 * D2
WINDOW, BIN = 300, 16


@pytest.fixture(scope="module")
def case(gpu_ctx):
    """An integer-valued movie (exact in uint16) whose level bleaches by 40 % over the recording, decomposed once, the
    fp32 denoised movie export_movie writes, and the emulated results of both kinds."""
    t = np.arange(T, dtype=np.float64)[:, None, None]
    mov = np.rint(8.0 * make_movie(T, D1, D2, seed=4) * (0.6 + 0.4 * np.exp(-t / 800.0))).astype(np.float32)
    np.random.seed(0)
    pmd = localmd_amd.localmd_decomposition(mov, (20, 20), 1000, max_components=4, background_rank=1, seed=3,
                                            sim_iters=5, order="F", ctx=gpu_ctx)
    den = np.empty((T, D1, D2), np.float32)
    localmd_amd.export_movie(pmd, den, panels="denoised", dtype="float32", ctx=gpu_ctx)
    h = R.half_of(WINDOW, BIN)
    ref = {kind: R.dff(y.reshape(T, D), BIN, h, "maximin", "dff") for kind, y in (("denoised", den), ("raw", mov))}
    return {"mov": mov, "pmd": pmd, "denoised": den.reshape(T, D), "raw": mov.reshape(T, D), "ref": ref, "h": h}


@pytest.mark.parametrize("kind", ["denoised", "raw"])
def test_rolling_baseline_knots_bit_for_bit(gpu_ctx, case, kind):
    y, pmd = case[kind], case["pmd"]
    assert y.min() > 0
    assert case["raw"][:200].mean() > 1.3 * case["raw"][-200:].mean()          # it bleaches
    for method in BL.METHODS:
        for b, window in ((BIN, WINDOW), (1, 41), (256, 1000)):
            bl = localmd_amd.rolling_baseline(pmd, case["mov"] if kind == "raw" else None, kind=kind, window=window,
                                              temporal_bin=b, method=method, ctx=gpu_ctx)
            h = R.half_of(window, b)
            want = R.filtered(R.movie_knots(y, b), h, method)
            assert bl.knots.shape == (-(-T // b), D1, D2) and bl.knots.dtype == np.float32
            assert bl.knots.reshape(-1, D).tobytes() == want.tobytes(), (method, b)
            assert (bl.temporal_bin, bl.window_frames, bl.method, bl.kind, bl.n_frames) == (b, (2 * h + 1) * b, method, kind, T)
            assert np.array_equal(bl.centres, R.centres(T, b))
    # the baseline follows the bleaching: the frames of the host evaluation against the emulation
    bl = pmd.baseline(case["mov"] if kind == "raw" else None, kind=kind, window=WINDOW, ctx=gpu_ctx)
    assert bl.temporal_bin == BIN and bl.knots.reshape(-1, D).tobytes() == case["ref"][kind][0].tobytes()
    F = bl.frames(1000, 1100).reshape(100, D)
    assert F.tobytes() == R.baseline_frames(case["ref"][kind][0], T, BIN, 1000, 1100).tobytes()
    if kind == "raw":
        assert bl.knots[:10].mean() > 1.2 * bl.knots[-10:].mean()             # and the baseline follows


@pytest.mark.parametrize("kind", ["denoised", "raw"])
def test_dff_movie_every_output_bit_for_bit(gpu_ctx, case, kind):
    y, pmd = case[kind], case["pmd"]
    movie = case["mov"] if kind == "raw" else None
    K = case["ref"][kind][0]
    F0 = R.baseline_frames(K, T, BIN, 0, T)
    bl = localmd_amd.rolling_baseline(pmd, movie, kind=kind, window=WINDOW, ctx=gpu_ctx)
    for output in BL.OUTPUTS:
        for min_baseline in ((0.0, float(np.median(K))) if output == "dff" else (0.0,)):
            out = np.full((T, D1, D2), POISON, np.float32)
            got = localmd_amd.dff_movie(pmd, out, movie, kind=kind, output=output, window=WINDOW,
                                        min_baseline=min_baseline, ctx=gpu_ctx)
            assert got is out
            want = R.outputs(y, F0, output, min_baseline)
            assert out.reshape(T, D).tobytes() == want.tobytes(), (output, min_baseline)
            if min_baseline:
                assert 0.2 < np.mean(out == 0) < 0.8
            two = np.empty((T, D1, D2), np.float32)
            pmd.dff(two, movie, kind=kind, output=output, baseline=bl, min_baseline=min_baseline, ctx=gpu_ctx)
            assert two.tobytes() == out.tobytes(), (output, min_baseline)
    assert case["ref"][kind][1].tobytes() == R.outputs(y, F0, "dff").tobytes()
    # another bin and the minimum alone
    out = np.empty((T, D1, D2), np.float32)
    localmd_amd.dff_movie(pmd, out, movie, kind=kind, output="detrended", window=500, temporal_bin=32, method="minimum",
                          ctx=gpu_ctx)
    assert out.reshape(T, D).tobytes() == R.dff(y, 32, R.half_of(500, 32), "minimum", "detrended")[1].tobytes()


class _Untouchable(lazy_data_loader):
    dtype = property(lambda self: np.float32)
    shape = property(lambda self: (T, D1, D2))

    def _compute_at_indices(self, indices):
        raise AssertionError("the movie was read")


class _Counting(lazy_data_loader):
    """A lazy uint16 movie over an array; counts how often every frame is served."""

    def __init__(self, a):
        self.a = a
        self.count = np.zeros(len(a), dtype=np.int64)

    dtype = property(lambda self: np.uint16)
    shape = property(lambda self: self.a.shape)

    def _compute_at_indices(self, indices):
        idx = np.arange(len(self.a))[indices].reshape(-1)
        np.add.at(self.count, idx, 1)
        return self.a[idx]


def test_invariance_over_batches_sources_destinations_and_residency(gpu_ctx, case, tmp_path):
    import torch

    pmd, mov = case["pmd"], case["mov"]
    want = {kind: case["ref"][kind][1].tobytes() for kind in ("denoised", "raw")}
    knots = {kind: case["ref"][kind][0].tobytes() for kind in ("denoised", "raw")}
    kw = dict(window=WINDOW, ctx=gpu_ctx)

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
    sources = {"numpy_u16": u16, "cpu_tensor": torch.from_numpy(mov), "device_tensor": torch.from_numpy(mov).to(gpu_ctx.device),
               "device_i16": torch.from_numpy(mov.astype(np.int16)).to(gpu_ctx.device)}
    for name, src in sources.items():
        assert run("raw", src, frame_batch_size=2048) == want["raw"], name
    # destinations
    for kind, movie in (("denoised", None), ("raw", u16)):
        npy = localmd_amd.dff_movie(pmd, str(tmp_path / (kind + ".npy")), movie, kind=kind, frame_batch_size=1024, **kw)
        assert np.load(npy).tobytes() == want[kind], kind
        tif = localmd_amd.dff_movie(pmd, str(tmp_path / (kind + ".tif")), movie, kind=kind, **kw)
        back = TiffArray(tif)
        assert back.dtype == np.float32 and np.asarray(back[:]).tobytes() == want[kind], kind
        dev = torch.full((T, D1, D2), float(POISON), dtype=torch.float32, device=gpu_ctx.device)
        assert localmd_amd.dff_movie(pmd, dev, movie, kind=kind, **kw) is dev
        assert dev.cpu().numpy().tobytes() == want[kind], kind
        cpu = torch.empty((T, D1, D2), dtype=torch.float32)
        localmd_amd.dff_movie(pmd, cpu, movie, kind=kind, **kw)
        assert cpu.numpy().tobytes() == want[kind], kind
    # device-resident factors
    pmd.to_device(ctx=gpu_ctx)
    try:
        out = np.empty((T, D1, D2), np.float32)
        pmd.dff(out, window=WINDOW)
        assert out.tobytes() == want["denoised"]
        assert pmd.baseline(u16, kind="raw", window=WINDOW).knots.tobytes() == knots["raw"]
    finally:
        pmd.to_host()


def test_movie_reads(gpu_ctx, case):
    """Denoised: the movie is never touched.  Raw: every frame once for the knots, twice for dff_movie, once with a
    given baseline."""
    pmd = case["pmd"]
    u16 = case["mov"].astype(np.uint16)
    out = np.empty((T, D1, D2), np.float32)
    localmd_amd.dff_movie(pmd, out, _Untouchable(), kind="denoised", window=WINDOW, ctx=gpu_ctx)
    assert out.reshape(T, D).tobytes() == case["ref"]["denoised"][1].tobytes()
    bl = localmd_amd.rolling_baseline(pmd, _Untouchable(), window=WINDOW, ctx=gpu_ctx)
    assert bl.knots.tobytes() == case["ref"]["denoised"][0].tobytes()
    src = _Counting(u16)
    bl = localmd_amd.rolling_baseline(pmd, src, kind="raw", window=WINDOW, frame_batch_size=1024, ctx=gpu_ctx)
    assert np.all(src.count == 1), np.unique(src.count)
    assert bl.knots.tobytes() == case["ref"]["raw"][0].tobytes()
    src = _Counting(u16)
    localmd_amd.dff_movie(pmd, out, src, kind="raw", window=WINDOW, frame_batch_size=1024, ctx=gpu_ctx)
    assert np.all(src.count == 2), np.unique(src.count)
    assert out.reshape(T, D).tobytes() == case["ref"]["raw"][1].tobytes()
    src = _Counting(u16)
    localmd_amd.dff_movie(pmd, out, src, kind="raw", baseline=bl, ctx=gpu_ctx)
    assert np.all(src.count == 1), np.unique(src.count)
    assert out.reshape(T, D).tobytes() == case["ref"]["raw"][1].tobytes()


def test_trace_baseline_equals_the_pixels_of_dff_movie(gpu_ctx, case):
    px = np.array([0, 1, 47, 48, 1000, D - 1])
    for kind in ("denoised", "raw"):
        y = case[kind]
        for output in BL.OUTPUTS:
            got = localmd_amd.trace_baseline(y[:, px].T, window=WINDOW, output=output, ctx=gpu_ctx)
            assert got.shape == (len(px), T) and got.dtype == np.float32 and got.flags.c_contiguous
            want = R.outputs(y, R.baseline_frames(case["ref"][kind][0], T, BIN, 0, T), output)[:, px].T
            assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (kind, output)
    one = localmd_amd.trace_baseline(case["raw"][:, 5].astype(np.uint16)[None, :], window=WINDOW, ctx=gpu_ctx)
    assert one.tobytes() == np.ascontiguousarray(case["ref"]["raw"][1][:, 5]).tobytes()


def test_opening_property_on_the_device(gpu_ctx):
    """test_baseline_host's opening property through trace_baseline: B[t] <= F0[t] <= B[t - L] away from the ends."""
    n, L, h = 4000, 20, 30
    t = np.arange(n)
    B = (100 * np.exp(-t / 800.0) + 50).astype(np.float32)
    x = np.stack([B, B])
    for s in range(100, n - 100, 150):
        x[1, s:s + L] += 40
    F0 = localmd_amd.trace_baseline(x, window=2 * h + 1, temporal_bin=1, output="baseline", ctx=gpu_ctx)
    inner = np.arange(2 * h, n - 2 * h)
    assert F0.tobytes() == R.filtered(x.T, h, "maximin").T.tobytes()
    assert np.all(B[inner] <= F0[1, inner]) and np.all(F0[1, inner] <= B[inner - L])
    assert np.array_equal(F0[0, inner], B[inner])                       # nothing to remove: the opening leaves B
    dff = localmd_amd.trace_baseline(x, window=2 * h + 1, temporal_bin=1, ctx=gpu_ctx)
    assert np.all(dff[1, inner] >= 0) and dff[1, 1000:1020].min() > 0.3 and np.abs(dff[0, inner]).max() == 0


def test_device_memory_grows_by_the_knot_terms_only(gpu_ctx):
    import torch

    d1 = d2 = 64
    peaks = {}
    for n in (8192, 16384):
        pmd = _long_pmd(n, d1, d2)
        gpu_ctx.release_workspace()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = np.empty((n, d1, d2), np.float32)
        localmd_amd.dff_movie(pmd, out, kind="denoised", window=WINDOW, frame_batch_size=4096, ctx=gpu_ctx)
        peaks[n] = torch.cuda.max_memory_allocated() - base
        assert np.all(np.isfinite(out))
    grow = BL.knot_bytes(16384, d1 * d2, 16) - BL.knot_bytes(8192, d1 * d2, 16)
    print("peak device bytes", peaks, "knot terms grow by", grow)
    assert grow == 3 * 4 * 512 * d1 * d2
    assert peaks[16384] - peaks[8192] <= grow, (peaks, grow)


def test_failed_export_removes_its_file(gpu_ctx, case, tmp_path):
    """A movie whose reader fails in the first pass, and one whose reader fails in the second: the error reaches the
    caller and the file is gone."""
    mov = case["mov"]

    class Failing(lazy_data_loader):
        dtype = property(lambda self: np.float32)
        shape = property(lambda self: mov.shape)

        def __init__(self, in_pass):
            self.in_pass, self.served = in_pass, 0

        def _compute_at_indices(self, indices):
            idx = np.arange(T)[indices].reshape(-1)
            self.served += len(idx)
            if idx.max() >= 2048 and self.served > (self.in_pass - 1) * T:
                raise OSError("read error")
            return mov[idx]

    for name in ("f.npy", "f.tif"):
        for in_pass in (1, 2):
            p = tmp_path / name
            src = Failing(in_pass)
            with pytest.raises(OSError):
                localmd_amd.dff_movie(case["pmd"], str(p), src, kind="raw", window=WINDOW, frame_batch_size=1024,
                                      ctx=gpu_ctx)
            assert not p.exists() and (src.served > T) == (in_pass == 2)
    assert not list(tmp_path.iterdir())
