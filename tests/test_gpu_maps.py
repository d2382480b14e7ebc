"""Regressor maps on the GPU (localmd_amd.regressor_maps, csrc/regress.hip): pmd_regress_accumulate through the C ABI
against fp64 NumPy (exactly for integer data, within the forward bound for float regressors), its bitwise independence of
K, of the leading dimensions and of the element type, the end-to-end bounds for sums, means and correlations of the raw /
denoised / residual movie, invariance over batch sizes, sources and device residency, a denoised-only call that reads no
movie, and a long uint16 movie mapped in one read with bounded device memory.

The fp64 references are formed here from the factors: X64 = mean + std * (U (R diag(s)) Vt), sums X Y64^T and X X64^T."""
import numpy as np
import pytest

import localmd_amd
from localmd_amd import decomposition as Dm
from localmd_amd import maps as MP
from localmd_amd._lib import PMDLibraryError, ptr
from localmd_amd._minitiff import write_tiff
from localmd_amd.dataset import TiffArray, lazy_data_loader
from localmd_amd.pmdarray import PMDArray, load_npz, save_npz
from localmd_amd.synthetic import make_movie
from tests.consumer_fuzz import check_sums, corr_bound as _corr_bound, den64 as _den64, factors64 as _factors64  # noqa: F401
from tests.consumer_fuzz import pearson64 as _pearson64, sum_bounds as _sum_bounds  # noqa: F401
from tests.test_export_host import _random_tiled_u
from tests.util import degenerate_pmds

pytestmark = pytest.mark.gpu
Dm.QUIET = True
T, D1, D2 = 2500, 40, 44
D = D1 * D2
ALL = ("denoised", "raw", "residual")
U24 = 2.0 ** -24
GAMMA = 1032 * U24
_ELEM = {"float32": 0, "uint16": 1, "int16": 2}


def _int_movie(seed):
    """Integer-valued fp32 movie (exact in uint16): mean about 900, noise std about 8."""
    return np.rint(8.0 * make_movie(T, D1, D2, seed=seed)).astype(np.float32)


def _decompose(ctx, mov, order, background_rank=1):
    np.random.seed(0)
    return localmd_amd.localmd_decomposition(mov, (20, 20), 1000, max_components=4, background_rank=background_rank,
                                             seed=3, sim_iters=5, order=order, ctx=ctx)


@pytest.fixture(scope="module")
def case(gpu_ctx):
    mov = _int_movie(4)
    return mov, {o: _decompose(gpu_ctx, mov, o) for o in ("F", "C")}


@pytest.fixture(scope="module")
def den64(case):
    return {o: _den64(p) for o, p in case[1].items()}


def _regressors(K, seed=7):
    return np.random.default_rng(seed).standard_normal((K, T))


# ---- the kernel through the C ABI ----------------------------------------------------------------------------------
def _dev(ctx, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _padded(a, ld, fill):
    out = np.full((a.shape[0], ld), fill, dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out


def _regress(ctx, Y, src, n, Dn, mean, X, K, *, ldx=None, lda=None, acc=None, want_mom=True, mom=None):
    """One pmd_regress_accumulate call on the first n rows of the host batch Y ((rows, ldy), any dtype; stored as
    ``src``).  Returns (acc (K, lda), mom (2 Dn,) or None) as NumPy; the paddings of X and acc are prefilled with NaN."""
    import torch

    y = _dev(ctx, Y.astype(src))
    ldy = Y.shape[1]
    ldx = n if ldx is None else ldx
    lda = Dn if lda is None else lda
    xd = _dev(ctx, _padded(np.asarray(X[:K, :n], np.float32), ldx, np.nan)) if K else None
    if acc is None:
        acc = _padded(np.zeros((K, Dn)), lda, np.nan)
    ad = _dev(ctx, acc) if K else None
    md = _dev(ctx, np.zeros(2 * Dn) if mom is None else mom) if want_mom else None
    ctx.call("pmd_regress_accumulate", ptr(y), _ELEM[src], ldy, n, Dn, ptr(None if mean is None else _dev(ctx, mean)),
             ptr(xd), ldx, K, ptr(ad), lda, ptr(md))
    ctx.sync()
    torch.cuda.synchronize()
    return (ad.cpu().numpy() if K else np.zeros((0, lda))), (md.cpu().numpy() if want_mom else None)


def test_kernel_exact_for_integer_data_every_container_length_and_K(gpu_ctx, case):
    mov = case[0]
    Yall = mov.reshape(T, D)
    assert mov.min() >= 0 and mov.max() <= 32767 and np.array_equal(mov, np.rint(mov))   # exact in all three containers
    mean = np.rint(Yall.astype(np.float64).mean(axis=0)).astype(np.float32)
    X = np.random.default_rng(11).integers(-2, 4, (70, 1024)).astype(np.float32)
    assert X.min() == -2 and X.max() == 3
    for b in range(0, T, 1024):         # the preconditions of exactness, on every 1024-frame block of the movie
        Zb = Yall[b:b + 1024].astype(np.float64) - mean
        assert (Zb * Zb).sum(axis=0).max() <= 3.2e6 and np.abs(Zb).sum(axis=0).max() <= 4.1e4
    assert 3.2e6 < 2 ** 24 and 3 * 4.1e4 < 2 ** 24                                        # every partial sum is an integer
    f0 = 1024
    Y = Yall[f0:f0 + 1024]
    Z = Y.astype(np.float64) - mean
    for n in (1, 2, 3, 63, 64, 65, 1024):
        want_mom = np.concatenate([Z[:n].sum(axis=0), (Z[:n] * Z[:n]).sum(axis=0)])
        for K in (1, 5, 32, 33, 70):
            want = X[:K, :n].astype(np.float64) @ Z[:n]
            for src in _ELEM:
                acc, mom = _regress(gpu_ctx, Y, src, n, D, mean, X, K)
                assert np.array_equal(acc, want), (n, K, src)
                assert np.array_equal(mom, want_mom), (n, K, src)
    # D = 37 pixels in rows of 41: a strip that ends inside a lane's run, rows that are not aligned
    Dn, ld = 37, 41
    for src, fill in (("float32", np.nan), ("uint16", 65535), ("int16", -32768)):
        Ys = _padded(Y[:, 100:100 + Dn].astype(src), ld, fill)
        for n, K in ((1, 1), (65, 33), (1024, 70)):
            acc, mom = _regress(gpu_ctx, Ys, src, n, Dn, mean[100:100 + Dn], X, K)
            Zs = Z[:n, 100:100 + Dn]
            assert np.array_equal(acc, X[:K, :n].astype(np.float64) @ Zs), (src, n, K)
            assert np.array_equal(mom, np.concatenate([Zs.sum(axis=0), (Zs * Zs).sum(axis=0)])), (src, n, K)
    # without a centring vector, and the moments alone
    acc, mom = _regress(gpu_ctx, Y, "uint16", 64, D, None, X, 5)
    Y64 = Y[:64].astype(np.float64)
    assert np.array_equal(acc, X[:5, :64].astype(np.float64) @ Y64)
    assert np.array_equal(mom[:D], Y64.sum(axis=0))
    y2 = (Y64 * Y64).sum(axis=0)                                 # 4e7: beyond 2^24, so within the forward bound only
    assert y2.max() > 2 ** 24 and np.all(np.abs(mom[D:] - y2) <= (64 + 8) * U24 * y2)
    _, mom = _regress(gpu_ctx, Y, "int16", 1024, D, mean, X, 0)
    assert np.array_equal(mom, np.concatenate([Z.sum(axis=0), (Z * Z).sum(axis=0)]))


def test_kernel_float_regressors_within_the_forward_bound(gpu_ctx, case):
    """|acc - acc64| <= (n + 8) 2^-24 (|X| |Z|): one rounding per product and per addition of the n-term chain, plus the
    roundings of the centring and of the regressor's conversion; the same form for the moments with |z| and z^2."""
    mov = case[0]
    Y = mov.reshape(T, D)[:1024]
    mean = Y.astype(np.float64).mean(axis=0).astype(np.float32)
    X = np.random.default_rng(12).standard_normal((70, 1024)).astype(np.float32)
    Z = Y.astype(np.float64) - mean.astype(np.float64)
    worst = 0.0
    for n in (1, 63, 65, 1024):
        for K in (5, 70):
            X64 = X[:K, :n].astype(np.float64)
            want, bound = X64 @ Z[:n], (n + 8) * U24 * (np.abs(X64) @ np.abs(Z[:n]))
            wm = np.concatenate([Z[:n].sum(axis=0), (Z[:n] * Z[:n]).sum(axis=0)])
            bm = (n + 8) * U24 * np.concatenate([np.abs(Z[:n]).sum(axis=0), (Z[:n] * Z[:n]).sum(axis=0)])
            got = {src: _regress(gpu_ctx, Y, src, n, D, mean, X, K) for src in _ELEM}
            acc, mom = got["float32"]
            ratio = max((np.abs(acc - want) / bound).max(), (np.abs(mom - wm) / bm).max())
            worst = max(worst, ratio)
            print("n", n, "K", K, "max error / bound", ratio)
            assert np.all(np.abs(acc - want) <= bound), (n, K, ratio)
            assert np.all(np.abs(mom - wm) <= bm), (n, K, ratio)
            for src in ("uint16", "int16"):
                assert got[src][0].tobytes() == acc.tobytes() and got[src][1].tobytes() == mom.tobytes(), (n, K, src)
    print("largest error / bound", worst)


def test_kernel_bits_do_not_depend_on_K_leading_dimensions_or_calls(gpu_ctx, case):
    mov = case[0]
    Yall = mov.reshape(T, D)
    mean = Yall.astype(np.float64).mean(axis=0).astype(np.float32)
    X = np.random.default_rng(13).standard_normal((70, 2048)).astype(np.float32)
    Y = Yall[:1024]
    n = 1001
    whole, mom = _regress(gpu_ctx, Y, "uint16", n, D, mean, X, 70)
    rows = np.concatenate([_regress(gpu_ctx, Y, "uint16", n, D, mean, X[a:b], b - a)[0] for a, b in
                           ((0, 1), (1, 33), (33, 70))])
    assert rows.tobytes() == whole.tobytes()
    # other leading dimensions (aligned rows, rows that are not): same bits, NaN paddings untouched
    for ldy, src in ((D + 8, "float32"), (D + 3, "uint16"), (D + 1, "float32")):
        Yp = _padded(Y, ldy, 7.0)
        acc, m2 = _regress(gpu_ctx, Yp, src, n, D, mean, X, 70, ldx=n + 5, lda=D + 6)
        assert acc[:, :D].tobytes() == np.ascontiguousarray(whole).tobytes() and m2.tobytes() == mom.tobytes(), ldy
        assert np.all(np.isnan(acc[:, D:]))
    # two consecutive calls add up in float64
    a1, m1 = _regress(gpu_ctx, Yall[:1024], "float32", 1024, D, mean, X[:, :1024], 70)
    a2, m2 = _regress(gpu_ctx, Yall[1024:2048], "float32", 1024, D, mean, X[:, 1024:], 70)
    both, mb = _regress(gpu_ctx, Yall[1024:2048], "float32", 1024, D, mean, X[:, 1024:], 70, acc=a1, mom=m1)
    assert np.array_equal(both, a1 + a2) and np.array_equal(mb, m1 + m2)


def test_kernel_rejects_bad_arguments(gpu_ctx):
    import torch

    buf = torch.zeros(4096, dtype=torch.float64, device=gpu_ctx.device)     # stands for every pointer: nothing launches
    p = ptr(buf)
    good = [p, 0, 35, 4, 35, p, p, 4, 2, p, 35, p]      # Y, elem, ldy, n, D, mean, X, ldx, K, acc, lda, mom

    def bad(**kw):
        names = ["Y", "elem", "ldy", "n", "D", "mean", "X", "ldx", "K", "acc", "lda", "mom"]
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        with pytest.raises(PMDLibraryError, match=r"failed \(-2\)"):      # PMD_ERR_ARG
            gpu_ctx.call("pmd_regress_accumulate", *a)

    bad(elem=7)
    bad(n=-1)
    bad(n=1025, ldx=1025)
    bad(D=0, ldy=0, lda=0)
    bad(K=-1)
    bad(ldy=34)
    bad(ldx=3)
    bad(lda=34)
    bad(Y=None)
    bad(X=None)
    bad(acc=None)
    # nothing to do: no pointer is looked at
    gpu_ctx.call("pmd_regress_accumulate", None, 0, 35, 0, 35, None, None, 0, 2, None, 35, None)
    gpu_ctx.call("pmd_regress_accumulate", None, 0, 35, 4, 35, None, None, 4, 0, None, 35, None)
    gpu_ctx.sync()
    assert float(buf.abs().sum()) == 0.0


# ---- end to end: sums and means ------------------------------------------------------------------------------------
def _check_sums(m, X64, Y64, X64den, absX, mean32, stat):
    check_sums(m, X64, Y64, X64den, absX, mean32, stat, D1, D2)


@pytest.mark.parametrize("stat", ["sum", "mean"])
@pytest.mark.parametrize("order", ["F", "C"])
def test_sums_and_means_against_fp64(gpu_ctx, case, den64, order, stat):
    mov, pmds = case
    pmd = pmds[order]
    Y64 = mov.reshape(T, D).astype(np.float64)
    X64den, absX = den64[order]
    mean32 = np.asarray(pmd.mean_img, np.float32).reshape(-1).astype(np.float64)
    X64 = _regressors(5)
    X64[4] = 1.0                                                  # a ones row: the sum image / the mean image
    m = localmd_amd.regressor_maps(pmd, X64, mov, kinds=ALL, stat=stat, frame_batch_size=1024, ctx=gpu_ctx)
    _check_sums(m, X64, Y64, X64den, absX, mean32, stat)
    if stat == "sum":
        # 0/1 regressors: the raw sums are integers below 2^24 and come out exactly
        B = (np.random.default_rng(3).random((3, T)) < 0.3).astype(np.float64)
        B[2] = 1.0
        want = B @ Y64
        assert want.max() < 2 ** 24
        mb = pmd.maps(B.astype(bool), mov.astype(np.uint16), kinds="raw", ctx=gpu_ctx)
        assert mb.denoised is None and mb.residual is None
        assert np.array_equal(mb.raw.reshape(3, D).astype(np.float64), want)
    else:
        # event-triggered average: the mean of the raw frames at event + lag
        events, lags = np.array([3, 500, 1023, 1024, 2400, 2499]), np.array([-4, 0, 1, 120])
        E = MP.event_regressors(T, events, lags)
        me = localmd_amd.regressor_maps(pmd, E, mov, kinds=ALL, stat="mean", ctx=gpu_ctx)
        _check_sums(me, E, Y64, X64den, absX, mean32, "mean")
        for row, lag in enumerate(lags):
            t = events + lag
            t = t[(t >= 0) & (t < T)]
            avg = Y64[t].mean(axis=0)
            bound = GAMMA * np.abs(Y64[t] - mean32[None, :]).mean(axis=0) + 2.0 ** -22 * np.abs(avg)
            assert np.all(np.abs(me.raw[row].reshape(-1) - avg) <= bound), lag


def test_background_rank_zero(gpu_ctx, case):
    mov = case[0]
    pmd = _decompose(gpu_ctx, mov, "F", background_rank=0)
    X64den, absX = _den64(pmd)
    mean32 = np.asarray(pmd.mean_img, np.float32).reshape(-1).astype(np.float64)
    X64 = _regressors(3, seed=9)
    Y64 = mov.reshape(T, D).astype(np.float64)
    for stat in ("sum", "mean"):
        m = localmd_amd.regressor_maps(pmd, X64, mov, kinds=ALL, stat=stat, ctx=gpu_ctx)
        _check_sums(m, X64, Y64, X64den, absX, mean32, stat)


# ---- end to end: correlation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["F", "C"])
def test_correlation_against_fp64_pearson(gpu_ctx, case, order):
    mov, pmds = case
    pmd = pmds[order]
    mean32 = np.asarray(pmd.mean_img, np.float32).reshape(-1)
    # the fp32 values the kernel sees: the raw frames minus the centring vector, the expanded denoised frames minus the
    # mean image, and the expanded residual frames
    panels = np.empty((T, D1, 2 * D2), np.float32)
    localmd_amd.export_movie(pmd, panels, mov, panels=("denoised", "residual"), ctx=gpu_ctx)
    Z = {"raw": (mov.reshape(T, D) - MP.centring_vector(pmd)[None, :]).astype(np.float64),
         "denoised": (np.ascontiguousarray(panels[:, :, :D2]).reshape(T, D) - mean32[None, :]).astype(np.float64),
         "residual": np.ascontiguousarray(panels[:, :, D2:]).reshape(T, D).astype(np.float64)}
    seed_px = 17 * D2 + 23
    traces = localmd_amd.extract_traces(pmd, np.eye(D, dtype=bool)[[seed_px, 5]].reshape(2, D1, D2), mov, kinds=ALL,
                                        reduce="sum", ctx=gpu_ctx)
    X64 = np.concatenate([_regressors(3, seed=21), mov[:, 17, 23][None, :].astype(np.float64),     # a pixel's own trace
                          traces.raw.astype(np.float64), traces.denoised[:1].astype(np.float64)])  # offsets near 900
    assert abs(X64[4].mean() - 900) < 100
    xhat = MP.normalized_regressors(X64).astype(np.float32).astype(np.float64)
    m = localmd_amd.regressor_maps(pmd, X64, mov, kinds=ALL, stat="correlation", frame_batch_size=2048, ctx=gpu_ctx)
    K = len(X64)
    for kind in ALL:
        got = getattr(m, kind)
        assert got.shape == (K, D1, D2) and got.dtype == np.float32
        r64, kappa = _pearson64(xhat, Z[kind])
        var = np.isfinite(kappa)                                 # pixels whose fp32 values vary at all
        assert var.sum() > 0.9 * D and np.all(got.reshape(K, D)[:, ~var] == 0)
        bound = _corr_bound(kappa[var])[None, :]
        err = np.abs(got.reshape(K, D)[:, var] - r64[:, var])
        print(order, kind, "kappa max", kappa[var].max(), "max error / bound", (err / bound).max())
        assert np.all(err <= bound), kind
        assert np.all(np.abs(got) <= 1.0)
    # the pixel's own trace, as given and as extract_traces returns it
    b = _corr_bound(_pearson64(xhat, Z["raw"])[1])[seed_px]
    assert m.raw[3, 17, 23] >= 1.0 - b and m.raw[4, 17, 23] >= 1.0 - b
    assert m.raw[3].tobytes() == m.raw[4].tobytes()
    # a constant pixel and a constant regressor correlate with nothing
    flat = mov.copy()
    flat[:, 7, 9] = 900.0
    Xc = np.concatenate([X64[:2], np.full((1, T), 3.5)])
    mc = localmd_amd.regressor_maps(pmd, Xc, flat.astype(np.uint16), kinds="raw", stat="correlation", ctx=gpu_ctx)
    assert np.array_equal(mc.raw[:, 7, 9], np.zeros(3, np.float32))
    assert np.array_equal(mc.raw[2], np.zeros((D1, D2), np.float32))
    keep = np.ones((D1, D2), bool)
    keep[7, 9] = False
    assert np.array_equal(mc.raw[:2][:, keep], m.raw[:2][:, keep])


@pytest.mark.parametrize("which", ["no_columns", "rank_zero"])
def test_decomposition_without_columns_or_rank(gpu_ctx, case, which):
    """The denoised movie is the mean image: its sums are mean sum x, it correlates with nothing, and the residual is
    the movie minus the mean image."""
    mov, pmds = case
    pmd = degenerate_pmds(pmds["C"])[which]
    X64den, absX = _den64(pmd)
    mean32 = np.asarray(pmd.mean_img, np.float32).reshape(-1)
    assert np.array_equal(X64den, np.repeat(mean32.astype(np.float64)[:, None], T, axis=1))
    X64 = _regressors(3, seed=5)
    m = localmd_amd.regressor_maps(pmd, X64, mov, kinds=ALL, stat="sum", frame_batch_size=1024, ctx=gpu_ctx)
    _check_sums(m, X64, mov.reshape(T, D).astype(np.float64), X64den, absX, mean32.astype(np.float64), "sum")
    m = localmd_amd.regressor_maps(pmd, X64, mov, kinds=ALL, stat="correlation", frame_batch_size=1024, ctx=gpu_ctx)
    assert np.array_equal(m.denoised, np.zeros((3, D1, D2), np.float32))
    Z = (mov.reshape(T, D) - mean32[None, :]).astype(np.float64)        # the fp32 residual frames
    xhat = MP.normalized_regressors(X64).astype(np.float32).astype(np.float64)
    r64, kappa = _pearson64(xhat, Z)
    var = np.isfinite(kappa)                                     # pixels whose fp32 values vary at all
    assert var.sum() > 0.9 * D and np.all(m.residual.reshape(3, D)[:, ~var] == 0)
    assert np.all(np.abs(m.residual.reshape(3, D)[:, var] - r64[:, var]) <= _corr_bound(kappa[var])[None, :])


# ---- invariance ----------------------------------------------------------------------------------------------------
def _bytes(m):
    return m.denoised.tobytes() + m.raw.tobytes() + m.residual.tobytes()


@pytest.mark.parametrize("stat", ["sum", "correlation"])
def test_batch_source_and_residency_invariance(gpu_ctx, case, tmp_path, stat):
    import torch

    mov, pmds = case
    pmd = pmds["F"]
    X = _regressors(4, seed=31)
    X[3] += 900.0
    kw = dict(kinds=ALL, stat=stat, ctx=gpu_ctx)
    want = _bytes(localmd_amd.regressor_maps(pmd, X, mov, frame_batch_size=1024, **kw))
    for fbs in (100, 1024, 10000):
        assert _bytes(localmd_amd.regressor_maps(pmd, X, mov, frame_batch_size=fbs, **kw)) == want, fbs
    u16 = mov.astype(np.uint16)
    mm = np.lib.format.open_memmap(str(tmp_path / "m.npy"), mode="w+", dtype=np.uint16, shape=mov.shape)
    mm[:] = u16
    path = str(tmp_path / "movie.tif")
    write_tiff(path, u16)
    sources = {"numpy_u16": u16, "memmap": mm, "cpu_tensor": torch.from_numpy(mov), "tiff": TiffArray(path),
               "device_tensor": torch.from_numpy(mov).to(gpu_ctx.device),
               "device_i16": torch.from_numpy(mov.astype(np.int16)).to(gpu_ctx.device)}
    for name, src in sources.items():
        assert _bytes(localmd_amd.regressor_maps(pmd, X, src, frame_batch_size=2048, **kw)) == want, name
    # kinds in another order, and one at a time
    got = localmd_amd.regressor_maps(pmd, X, mov, kinds=("residual", "raw", "denoised"), stat=stat, ctx=gpu_ctx)
    assert _bytes(got) == want
    for kind in ALL:
        one = localmd_amd.regressor_maps(pmd, X, u16, kinds=kind, stat=stat, frame_batch_size=1024, ctx=gpu_ctx)
        assert [k for k in ALL if getattr(one, k) is not None] == [kind]
        assert getattr(one, kind).tobytes() == getattr(got, kind).tobytes(), kind
    # device-resident factors
    pmd.to_device(ctx=gpu_ctx)
    try:
        got = pmd.maps(X, mov, kinds=ALL, stat=stat)
    finally:
        pmd.to_host()
    assert _bytes(got) == want
    # a decomposition read back from disk, and the method against the function
    npz = str(tmp_path / "pmd.npz")
    save_npz(npz, pmd)
    assert _bytes(localmd_amd.regressor_maps(load_npz(npz), X, mov, **kw)) == want
    assert _bytes(pmd.maps(X, mov, **kw)) == want
    # one regressor as (T,), and the rows on their own
    one = localmd_amd.regressor_maps(pmd, X[2], mov, **kw)
    assert one.raw.shape == (1, D1, D2)
    if stat == "sum":
        full = localmd_amd.regressor_maps(pmd, X, mov, **kw)
        assert one.raw.tobytes() == full.raw[2:3].tobytes()


class _Untouchable(lazy_data_loader):
    dtype = property(lambda self: np.float32)
    shape = property(lambda self: (T, D1, D2))

    def _compute_at_indices(self, indices):
        raise AssertionError("the movie was read")


@pytest.mark.parametrize("stat", ["sum", "mean"])
def test_denoised_only_reads_no_movie(gpu_ctx, case, stat):
    mov, pmds = case
    pmd = pmds["C"]
    X = 1.0 + _regressors(3, seed=41)
    a = localmd_amd.regressor_maps(pmd, X, stat=stat, ctx=gpu_ctx)                  # kinds defaults to "denoised"
    b = localmd_amd.regressor_maps(pmd, X, _Untouchable(), kinds=("denoised",), stat=stat, ctx=gpu_ctx)
    c = localmd_amd.regressor_maps(pmd, X, mov, kinds=ALL, stat=stat, ctx=gpu_ctx)
    assert a.raw is None and a.residual is None and b.raw is None
    assert a.denoised.tobytes() == b.denoised.tobytes() == c.denoised.tobytes()


# ---- a long movie --------------------------------------------------------------------------------------------------
class _CountingU16(lazy_data_loader):
    """Lazy uint16 movie generated on the fly; counts how often every frame is served."""

    def __init__(self, n, d1, d2):
        self._shape = (n, d1, d2)
        self.noise = np.random.default_rng(5).integers(0, 200, (64, d1, d2)).astype(np.uint16)
        self.count = np.zeros(n, dtype=np.int64)

    dtype = property(lambda self: np.uint16)
    shape = property(lambda self: self._shape)

    def frames(self, idx):
        return (self.noise[(idx * 7919) % 64] + (idx % 1000)[:, None, None].astype(np.uint16)).astype(np.uint16)

    def _compute_at_indices(self, indices):
        idx = np.arange(self._shape[0])[indices].reshape(-1)
        np.add.at(self.count, idx, 1)
        return self.frames(idx)


def _long_pmd(n, d1, d2):
    u = _random_tiled_u(d1, d2, 32, 32, "F", 2, seed=4)
    rng = np.random.default_rng(6)
    k = u.shape[1]
    rank = 12
    return PMDArray(u, rng.standard_normal((k, rank)) * 0.1, np.linspace(20, 2, rank), rng.standard_normal((rank, n)) * 0.01,
                    (n, d1, d2), "F", rng.uniform(500, 1500, (d1, d2)), rng.uniform(2, 10, (d1, d2)))


def test_long_movie_read_once_bounded_memory(gpu_ctx):
    import torch

    d1 = d2 = 64
    px = [(0, 0), (31, 40), (63, 63)]
    peaks = {}
    for n in (8000, 40000):
        src = _CountingU16(n, d1, d2)
        pmd = _long_pmd(n, d1, d2)
        X = np.random.default_rng(9).standard_normal((4, n))
        gpu_ctx.release_workspace()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        m = localmd_amd.regressor_maps(pmd, X, src, kinds=ALL, stat="correlation", frame_batch_size=4096, ctx=gpu_ctx)
        peaks[n] = torch.cuda.max_memory_allocated() - base
        assert np.all(src.count == 1), np.unique(src.count)
        t = np.arange(n)
        xhat = MP.normalized_regressors(X).astype(np.float32).astype(np.float64)
        centre = MP.centring_vector(pmd).reshape(d1, d2)
        for i, j in px:
            y = (src.noise[(t * 7919) % 64, i, j].astype(np.float32) + (t % 1000).astype(np.float32))
            z = (y - centre[i, j]).astype(np.float64)[:, None]
            r64, kappa = _pearson64(xhat, z)
            assert np.all(np.abs(m.raw[:, i, j] - r64[:, 0]) <= _corr_bound(kappa)[0]), (n, i, j)
        assert np.all(np.isfinite(m.denoised)) and np.all(np.isfinite(m.residual))
    print("peak device bytes", peaks)
    assert peaks[40000] <= peaks[8000], peaks
