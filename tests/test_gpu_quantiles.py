"""Quantile images on the GPU (localmd_amd.quantile_images, csrc/quantile.hip): the full pass sequence of
pmd_pixel_hist_accumulate / pmd_pixel_hist_select through the C ABI against np.sort (exactly, for every element type,
with and without a centring vector, whole batches and split ones, padded and unaligned rows, ties, constant pixels, keys
that differ in the last digit or the sign only, infinities and NaN), bad arguments; end to end every kind, position and
interpolation against np.sort of the exported movie bit for bit, the MAD, q = 0 / 1 against summary_images, invariance
over batch sizes, sources, residency, kinds and q, a denoised-only call that reads no movie, the documented number of
passes over a lazily generated movie, and device memory that does not grow with its length.

The referee throughout is np.sort along time on the float32 movie."""
import numpy as np
import pytest

import localmd_amd
from localmd_amd import decomposition as Dm
from localmd_amd import quantiles as QT
from localmd_amd._lib import PMDLibraryError, ptr
from localmd_amd._minitiff import write_tiff
from localmd_amd.dataset import TiffArray, lazy_data_loader
from tests.consumer_fuzz import exported as _exported, mad_reference as _mad_reference, quantile_reference as _reference
from tests.test_gpu_maps import _CountingU16, _decompose, _int_movie, _long_pmd
from tests.util import degenerate_pmds

pytestmark = pytest.mark.gpu
Dm.QUIET = True
T, D1, D2 = 2500, 40, 44
D = D1 * D2
ALL = ("denoised", "raw", "residual")
_ELEM = {"float32": 0, "uint16": 1, "int16": 2}
_FILL = {"float32": np.nan, "uint16": 65535, "int16": -32768}      # paddings of Y: they would show up
DS = (63, 65, 129, D)
NS = (1, 3, 257, 1030)
QS = (0.0, 0.08, 0.5, 1.0)


# ---- the kernels through the C ABI ---------------------------------------------------------------------------------
def _dev(ctx, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _padded(a, ld, src):
    out = np.full((a.shape[0], ld), _FILL[src], dtype=src)
    out[:, :a.shape[1]] = a
    return out


def _splits(n, parts):
    cuts = sorted({0, n} | {n * i // parts for i in range(1, parts)})
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def _select(ctx, yd, src, ldy, n, Dn, rank, centre=None, parts=1, passes=4):
    """The order statistic ``rank`` of the first n rows of the device batch yd (rows of ldy elements of type ``src``):
    ``passes`` passes of accumulate (one call per part of the batch) and select.  Returns the (Dn,) float32 values; checks
    that the histogram is left zero and the rank within range."""
    import ctypes as C
    import torch

    G = -(-Dn // 64)
    hist = torch.zeros(G * 256 * 64, dtype=torch.int32, device=ctx.device)
    rk = torch.full((Dn,), int(rank), dtype=torch.int32, device=ctx.device)
    prefix = torch.zeros(Dn, dtype=torch.int32, device=ctx.device)
    cd = None if centre is None else _dev(ctx, np.asarray(centre, np.float32))
    for p in range(passes):
        for a, b in _splits(n, parts):
            yp = C.c_void_p(yd.data_ptr() + a * ldy * yd.element_size())
            ctx.call("pmd_pixel_hist_accumulate", yp, _ELEM[src], ldy, b - a, Dn, ptr(cd), p, ptr(prefix), ptr(hist))
        ctx.call("pmd_pixel_hist_select", Dn, ptr(hist), ptr(rk), ptr(prefix))
    ctx.sync()
    assert not bool(hist.any()) and int(rk.min()) >= 0 and int(rk.max()) <= rank
    k = prefix.cpu().numpy().view(np.uint32)
    if passes == 3:                                  # 16-bit integers: the last digit is 0x00, or 0xFF under a negative value
        k = (k << np.uint32(8)) | np.where(k & np.uint32(0x800000), np.uint32(0), np.uint32(0xFF))
    return QT.key_floats(k)


def _ranks(n):
    return sorted({0, (n - 1) // 2, n // 2, n - 1})


@pytest.mark.parametrize("Dn", DS)
def test_kernel_integer_data_every_container_length_split_and_rank(gpu_ctx, Dn):
    """Values 0..6 (ties everywhere) and one constant pixel: np.sort exactly, the same bits for the three containers,
    with and without a centring vector (|y - centre| in fp32), paddings of 65535 / NaN / -32768 never counted."""
    rng = np.random.default_rng(1)
    Y = rng.integers(0, 7, (max(NS), Dn))
    Y[:, Dn // 2] = 5
    centre = rng.choice(np.array([3.0, 2.5, 0.25, 100.0], np.float32), Dn)
    y32 = Y.astype(np.float32)
    for ldy in (Dn, Dn + 3):
        dev = {src: _dev(gpu_ctx, _padded(Y, ldy, src)) for src in _ELEM}
        for n in NS:
            plain = np.sort(y32[:n], axis=0)
            centred = np.sort(np.abs(y32[:n] - centre[None, :]), axis=0)
            for parts in (1, 3):
                for r in _ranks(n):
                    first = None
                    for src in _ELEM:
                        key = (Dn, ldy, n, parts, r, src)
                        got = _select(gpu_ctx, dev[src], src, ldy, n, Dn, r, None, parts)
                        assert got.tobytes() == plain[r].tobytes(), key
                        gc = _select(gpu_ctx, dev[src], src, ldy, n, Dn, r, centre, parts)
                        assert gc.tobytes() == centred[r].tobytes(), key
                        first = got.tobytes() + gc.tobytes() if first is None else first
                        assert got.tobytes() + gc.tobytes() == first, key
            # the last digit of a 16-bit integer's key is known: three passes give the upper 24 bits
            for src in ("uint16", "int16"):
                got = _select(gpu_ctx, dev[src], src, ldy, n, Dn, n // 2, None, 3, passes=3)
                assert got.tobytes() == plain[n // 2].tobytes(), (Dn, ldy, n, src)
    # int16 with negative values
    Yn = rng.integers(-300, 300, (257, Dn)).astype(np.int16)
    want = np.sort(Yn.astype(np.float32), axis=0)
    yd = _dev(gpu_ctx, _padded(Yn, Dn + 3, "int16"))
    for r in _ranks(257):
        assert _select(gpu_ctx, yd, "int16", Dn + 3, 257, Dn, r).tobytes() == want[r].tobytes(), r


def _float_case(n, Dn, rng):
    """(n, Dn) float32: noise, and columns whose keys differ in the last digit only (neighbours of 1), in the sign only,
    +-inf, one NaN, +-0, denormals, and a constant."""
    one = np.float32(1.0)
    near = np.array([np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(2))], np.float32)
    Y = (900.0 + 8.0 * rng.standard_normal((n, Dn))).astype(np.float32)
    Y[:, 0] = near[rng.integers(0, 3, n)]
    Y[:, 1] = rng.choice(np.array([-3.5, 3.5], np.float32), n)
    Y[:, 2] = rng.choice(np.array([-np.inf, -1.0, 2.0, np.inf], np.float32), n)
    Y[n // 2, 3] = np.nan
    Y[:, 4] = np.float32(1e-39) * rng.integers(-5, 6, n).astype(np.float32)      # denormals of both signs
    Y[:, 5] = 7.25
    Y[:, Dn - 1] = near[rng.integers(0, 3, n)]                                      # the last pixel of a ragged group
    return Y


@pytest.mark.parametrize("Dn", DS)
def test_kernel_float_data_last_digit_sign_inf_nan_and_denormals(gpu_ctx, Dn):
    rng = np.random.default_rng(2)
    for n in NS:
        Y = _float_case(n, Dn, rng)
        centre = (900.0 + rng.standard_normal(Dn)).astype(np.float32)
        centre[0] = centre[Dn - 1] = 1.0                       # differences of one and two ulps of 1, and 0
        centre[1], centre[2], centre[3] = 3.5, 0.5, 0.0
        centre[4] = np.float32(2e-39)                          # denormal differences: not flushed
        centre[5] = 7.25
        plain = np.sort(Y, axis=0)
        with np.errstate(invalid="ignore"):
            centred = np.sort(np.abs(Y - centre[None, :]), axis=0)
        if n >= 257:
            assert np.any((centred[:, 4] > 0) & (centred[:, 4] < np.finfo(np.float32).tiny))
        for ldy in (Dn, Dn + 3):
            yd = _dev(gpu_ctx, _padded(Y, ldy, "float32"))
            for parts in (1, 3):
                for r in _ranks(n):
                    key = (Dn, ldy, n, parts, r)
                    got = _select(gpu_ctx, yd, "float32", ldy, n, Dn, r, None, parts)
                    assert np.array_equal(got, plain[r], equal_nan=True), key
                    keep = ~np.isnan(plain[r]) & (plain[r] != 0)                    # the bits, where np.sort fixes them
                    assert got[keep].tobytes() == plain[r][keep].tobytes(), key
                    gc = _select(gpu_ctx, yd, "float32", ldy, n, Dn, r, centre, parts)
                    assert np.array_equal(gc, centred[r], equal_nan=True), key
                    assert gc[~np.isnan(gc)].tobytes() == centred[r][~np.isnan(centred[r])].tobytes(), key


def test_kernel_counts_every_element_once_and_no_padding(gpu_ctx):
    """After the first pass the counts of every pixel add up to n, bin by bin those of NumPy; pixels beyond D in the last
    group hold nothing; minus zero is counted below plus zero."""
    import torch

    rng = np.random.default_rng(3)
    n, Dn, ldy = 1030, 129, 132
    Y = _float_case(n, Dn, rng)
    Y[:, 6] = rng.choice(np.array([-0.0, 0.0], np.float32), n)
    G = -(-Dn // 64)
    hist = torch.zeros((G, 256, 64), dtype=torch.int32, device=gpu_ctx.device)
    yd = _dev(gpu_ctx, _padded(Y, ldy, "float32"))
    gpu_ctx.call("pmd_pixel_hist_accumulate", ptr(yd), 0, ldy, n, Dn, None, 0, None, ptr(hist))
    gpu_ctx.sync()
    h = hist.cpu().numpy().transpose(0, 2, 1).reshape(G * 64, 256)
    assert np.all(h[:Dn].sum(axis=1) == n) and not h[Dn:].any()
    digits = (QT.float_keys(Y) >> np.uint32(24)).astype(np.int64)
    want = np.stack([np.bincount(digits[:, c], minlength=256) for c in range(Dn)])
    assert np.array_equal(h[:Dn], want)
    assert h[6, 0x7F] == int(np.signbit(Y[:, 6]).sum()) and h[6, 0x80] == n - h[6, 0x7F]
    assert h[3, 0xFF] == 1                                             # the NaN
    # a second call adds to the counts; select on the sign column finds -0 below +0
    gpu_ctx.call("pmd_pixel_hist_accumulate", ptr(yd), 0, ldy, n, Dn, None, 0, None, ptr(hist))
    gpu_ctx.sync()
    assert np.array_equal(hist.cpu().numpy().transpose(0, 2, 1).reshape(G * 64, 256)[:Dn], 2 * want)
    zeros = int(np.signbit(Y[:, 6]).sum())
    assert 0 < zeros < n
    lo = _select(gpu_ctx, yd, "float32", ldy, n, Dn, zeros - 1)[6]
    hi = _select(gpu_ctx, yd, "float32", ldy, n, Dn, zeros)[6]
    assert lo == 0 and hi == 0 and np.signbit(lo) and not np.signbit(hi)


def test_kernels_reject_bad_arguments(gpu_ctx):
    import torch

    Dn = 35
    y = torch.ones((8, 40), dtype=torch.float32, device=gpu_ctx.device)
    hist = torch.zeros(256 * 64 + 4, dtype=torch.int32, device=gpu_ctx.device)
    rank = torch.full((Dn,), 2, dtype=torch.int32, device=gpu_ctx.device)
    prefix = torch.zeros(Dn, dtype=torch.int32, device=gpu_ctx.device)
    centre = torch.zeros(Dn, dtype=torch.float32, device=gpu_ctx.device)
    names = ["Y", "elem", "ldy", "n", "D", "centre", "pass", "prefix", "hist"]
    good = [ptr(y), 0, 40, 4, Dn, ptr(centre), 0, ptr(prefix), ptr(hist)]

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        with pytest.raises(PMDLibraryError, match=r"failed \(-2\)"):      # PMD_ERR_ARG
            gpu_ctx.call("pmd_pixel_hist_accumulate", *a)

    bad(n=0)
    bad(n=-1)
    bad(n=2 ** 31)
    bad(D=0, ldy=0)
    bad(ldy=Dn - 1)
    bad(elem=7)
    bad(elem=-1)
    bad(**{"pass": 4})
    bad(**{"pass": -1})
    bad(**{"pass": 1}, prefix=None)
    bad(Y=None)
    bad(hist=None)
    bad(hist=ptr(hist[1:]))                                              # not 16-byte aligned
    for a in ((0, ptr(hist), ptr(rank), ptr(prefix)), (-3, ptr(hist), ptr(rank), ptr(prefix)),
              (Dn, None, ptr(rank), ptr(prefix)), (Dn, ptr(hist), None, ptr(prefix)), (Dn, ptr(hist), ptr(rank), None)):
        with pytest.raises(PMDLibraryError, match=r"failed \(-2\)"):
            gpu_ctx.call("pmd_pixel_hist_select", *a)
    gpu_ctx.sync()
    assert not bool(hist.any()) and not bool(prefix.any()) and bool((rank == 2).all())
    # and a good call afterwards works: four frames of ones, rank 2 -> 1.0
    assert np.array_equal(_select(gpu_ctx, y, "float32", 40, 4, Dn, 2), np.ones(Dn, np.float32))
    gpu_ctx.call("pmd_pixel_hist_accumulate", *good)
    gpu_ctx.call("pmd_pixel_hist_accumulate", ptr(y), 0, 40, 4, Dn, None, 0, None, ptr(hist))       # pass 0 needs no prefix
    gpu_ctx.sync()
    assert int(hist.sum()) == 2 * 4 * Dn


# ---- end to end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(gpu_ctx):
    """The movie, its decompositions and, once for the module, np.sort of the exported fp32 panels of order "F"."""
    mov = _int_movie(4)
    pmds = {o: _decompose(gpu_ctx, mov, o) for o in ("F", "C")}
    return mov, pmds


@pytest.fixture(scope="module")
def sorted_panels(gpu_ctx, case):
    mov, pmds = case
    out = {}
    for o, pmd in pmds.items():
        panels = _exported(gpu_ctx, pmd, mov)
        assert np.array_equal(panels["raw"], mov.reshape(T, D))
        out[o] = (panels, {k: np.sort(v, axis=0) for k, v in panels.items()})
    return out


@pytest.mark.parametrize("order", ["F", "C"])
def test_every_kind_position_and_interpolation_against_np_sort(gpu_ctx, case, sorted_panels, order):
    mov, pmds = case
    pmd = pmds[order]
    panels, S = sorted_panels[order]
    assert int(np.floor(0.08 * (T - 1))) == 199 and 0.5 * (T - 1) == 1249.5
    for interpolation in QT.INTERPOLATIONS:
        r = localmd_amd.quantile_images(pmd, mov, kinds=ALL, q=QS, interpolation=interpolation, frame_batch_size=1024,
                                        ctx=gpu_ctx)
        assert r.q == QS and r.interpolation == interpolation and r.mad is None
        for kind in ALL:
            got = getattr(r, kind)
            assert got.shape == (len(QS), D1, D2) and got.dtype == np.float32
            assert got.tobytes() == _reference(S[kind], QS, interpolation).tobytes(), (interpolation, kind)
    # the median against NumPy's own, on the integer movie (exact in both)
    med = localmd_amd.quantile_images(pmd, mov.astype(np.uint16), kinds="raw", ctx=gpu_ctx)
    assert med.q == (0.5,) and med.raw.shape == (1, D1, D2) and med.denoised is None and med.residual is None
    assert np.array_equal(med.raw[0], np.median(mov, axis=0))
    # q = 0 and q = 1 are the extrema of summary_images
    s = localmd_amd.summary_images(pmd, mov, kinds=ALL, stats=("min", "max"), ctx=gpu_ctx)
    ends = localmd_amd.quantile_images(pmd, mov, kinds=ALL, q=(0, 1), interpolation="lower", ctx=gpu_ctx)
    for kind in ALL:
        assert getattr(ends, kind)[0].tobytes() == getattr(s, kind)["min"].tobytes(), kind
        assert getattr(ends, kind)[1].tobytes() == getattr(s, kind)["max"].tobytes(), kind


def test_mad_against_np_sort(gpu_ctx, case, sorted_panels):
    mov, pmds = case
    panels, S = sorted_panels["F"]
    r = localmd_amd.quantile_images(pmds["F"], mov, kinds=ALL, q=(0.08, 0.5), mad=True, ctx=gpu_ctx)
    assert sorted(r.mad) == sorted(ALL)
    for kind in ALL:
        assert getattr(r, kind).tobytes() == _reference(S[kind], (0.08, 0.5), "linear").tobytes(), kind
        got = r.mad[kind]
        assert got.shape == (D1, D2) and got.dtype == np.float32
        assert got.tobytes() == _mad_reference(panels[kind], S[kind]).reshape(D1, D2).tobytes(), kind
    # the noise of this movie has std about 8: the scaled MAD of the residual is near it
    sigma = QT.MAD_TO_STD * r.mad["residual"]
    assert 4.0 < float(np.median(sigma)) < 12.0
    assert repr(r) == "Quantiles(denoised, raw, residual; q=(0.08, 0.5); linear; mad)"


# ---- invariance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["no_columns", "rank_zero"])
def test_decomposition_without_columns_or_rank(gpu_ctx, case, which):
    """The denoised movie is the mean image in every frame; quantiles and MAD against np.sort of the exported panels."""
    mov, pmds = case
    pmd = degenerate_pmds(pmds["F"])[which]
    panels = _exported(gpu_ctx, pmd, mov)
    mean32 = np.asarray(pmd.mean_img, np.float32).reshape(-1)
    assert np.array_equal(panels["denoised"], np.broadcast_to(mean32, (T, D)))
    assert np.array_equal(panels["residual"], mov.reshape(T, D) - mean32[None, :])
    r = localmd_amd.quantile_images(pmd, mov, kinds=ALL, q=(0.08, 0.5), mad=True, frame_batch_size=1024, ctx=gpu_ctx)
    for kind in ALL:
        S = np.sort(panels[kind], axis=0)
        assert getattr(r, kind).tobytes() == _reference(S, (0.08, 0.5), "linear").tobytes(), kind
        assert r.mad[kind].tobytes() == _mad_reference(panels[kind], S).reshape(D1, D2).tobytes(), kind
    assert not r.mad["denoised"].any()


def _bytes(r, kinds=ALL):
    return b"".join(getattr(r, k).tobytes() + r.mad[k].tobytes() for k in kinds)


class _Lazy(lazy_data_loader):
    def __init__(self, a):
        self.a = a

    dtype = property(lambda self: self.a.dtype)
    shape = property(lambda self: self.a.shape)

    def _compute_at_indices(self, indices):
        return self.a[indices]


def test_batch_source_kind_q_and_residency_invariance(gpu_ctx, case, tmp_path):
    import torch

    mov, pmds = case
    pmd = pmds["F"]
    kw = dict(kinds=ALL, q=QS, mad=True, ctx=gpu_ctx)
    ref = localmd_amd.quantile_images(pmd, mov, frame_batch_size=1024, **kw)
    want = _bytes(ref)
    for fbs in (300, 1024, 10000):
        assert _bytes(localmd_amd.quantile_images(pmd, mov, frame_batch_size=fbs, **kw)) == want, fbs
    u16 = mov.astype(np.uint16)
    path = str(tmp_path / "movie.tif")
    write_tiff(path, u16)
    sources = {"numpy_u16": u16, "tiff": TiffArray(path), "device_tensor": torch.from_numpy(mov).to(gpu_ctx.device),
               "device_i16": torch.from_numpy(mov.astype(np.int16)).to(gpu_ctx.device), "lazy_u16": _Lazy(u16),
               "lazy_f32": _Lazy(mov)}
    for name, src in sources.items():
        assert _bytes(localmd_amd.quantile_images(pmd, src, frame_batch_size=2048, **kw)) == want, name
    # kinds in another order and one at a time (a 16-bit raw movie alone takes the three-pass route)
    got = localmd_amd.quantile_images(pmd, mov, kinds=("residual", "raw", "denoised"), q=QS, mad=True, ctx=gpu_ctx)
    assert _bytes(got) == want
    for kind in ALL:
        for src in (u16, mov):
            one = localmd_amd.quantile_images(pmd, src, kinds=kind, q=QS, mad=True, frame_batch_size=1024, ctx=gpu_ctx)
            assert [k for k in ALL if getattr(one, k) is not None] == [kind] and sorted(one.mad) == [kind]
            assert _bytes(one, (kind,)) == _bytes(ref, (kind,)), kind
    raw3 = localmd_amd.quantile_images(pmd, u16, kinds=("raw", "denoised"), q=QS, ctx=gpu_ctx)
    assert raw3.raw.tobytes() == ref.raw.tobytes() and raw3.denoised.tobytes() == ref.denoised.tobytes()
    # q in another order, with duplicates, and one at a time
    perm = (1.0, 0.5, 0.5, 0.0, 0.08)
    got = localmd_amd.quantile_images(pmd, mov, kinds=ALL, q=perm, ctx=gpu_ctx)
    for kind in ALL:
        for i, x in enumerate(perm):
            assert getattr(got, kind)[i].tobytes() == getattr(ref, kind)[QS.index(x)].tobytes(), (kind, x)
    for i, x in enumerate(QS):
        one = localmd_amd.quantile_images(pmd, mov, kinds=ALL, q=x, ctx=gpu_ctx)
        for kind in ALL:
            assert getattr(one, kind).shape == (1, D1, D2)
            assert getattr(one, kind)[0].tobytes() == getattr(ref, kind)[i].tobytes(), (kind, x)
    # device-resident factors, and the method against the function
    pmd.to_device(ctx=gpu_ctx)
    try:
        got = pmd.quantiles(mov, kinds=ALL, q=QS, mad=True)
    finally:
        pmd.to_host()
    assert _bytes(got) == want
    assert _bytes(pmd.quantiles(mov, **kw)) == want


class _Untouchable(lazy_data_loader):
    dtype = property(lambda self: np.float32)
    shape = property(lambda self: (T, D1, D2))

    def _compute_at_indices(self, indices):
        raise AssertionError("the movie was read")


def test_denoised_only_reads_no_movie(gpu_ctx, case, sorted_panels):
    mov, pmds = case
    pmd = pmds["C"]
    a = localmd_amd.quantile_images(pmd, ctx=gpu_ctx)                     # kinds "denoised", q 0.5
    b = localmd_amd.quantile_images(pmd, _Untouchable(), kinds=("denoised",), mad=True, ctx=gpu_ctx)
    c = localmd_amd.quantile_images(pmd, mov, kinds=ALL, ctx=gpu_ctx)
    assert a.q == (0.5,) and a.raw is None and a.residual is None and b.raw is None and a.mad is None
    assert a.denoised.tobytes() == b.denoised.tobytes() == c.denoised.tobytes()
    assert a.denoised[0].reshape(-1).tobytes() == _reference(sorted_panels["C"][1]["denoised"], (0.5,), "linear")[0].tobytes()
    assert sorted(b.mad) == ["denoised"]


# ---- a long movie --------------------------------------------------------------------------------------------------
def test_long_movie_pass_counts_and_bounded_memory(gpu_ctx):
    import torch

    d1 = d2 = 64
    px = [(0, 0), (31, 40), (63, 63)]
    peaks = {}
    for n in (5000, 10000):
        pmd = _long_pmd(n, d1, d2)
        src = _CountingU16(n, d1, d2)
        gpu_ctx.release_workspace()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        r = localmd_amd.quantile_images(pmd, src, kinds=ALL, q=(0.08, 0.5), mad=True, frame_batch_size=2048, ctx=gpu_ctx)
        peaks[n] = torch.cuda.max_memory_allocated() - base
        assert QT.movie_passes(2, ALL, mad=True) == 8
        assert np.all(src.count == 8), np.unique(src.count)           # four passes for the quantiles, four for the MAD
        t = np.arange(n)
        for i, j in px:
            y = np.sort(src.noise[(t * 7919) % 64, i, j].astype(np.float32) + (t % 1000).astype(np.float32))[:, None]
            assert np.array_equal(r.raw[:, i, j], _reference(y, (0.08, 0.5), "linear")[:, 0]), (n, i, j)
        for kind in ALL:
            assert np.all(np.isfinite(getattr(r, kind))) and np.all(np.isfinite(r.mad[kind])), kind
    print("peak device bytes", peaks)
    assert peaks[10000] <= peaks[5000], peaks
    # a 16-bit movie on its own: three passes, four more for the MAD; next to the denoised kind as well
    n = 3000
    pmd = _long_pmd(n, d1, d2)
    for kinds, mad, passes in (("raw", False, 3), (("denoised", "raw"), False, 3), ("raw", True, 7)):
        src = _CountingU16(n, d1, d2)
        localmd_amd.quantile_images(pmd, src, kinds=kinds, q=0.08, mad=mad, frame_batch_size=2048, ctx=gpu_ctx)
        assert QT.movie_passes(2, kinds, mad=mad) == passes
        assert np.all(src.count == passes), (kinds, mad, np.unique(src.count))
