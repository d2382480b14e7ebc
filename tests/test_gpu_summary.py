"""Summary images on the GPU (localmd_amd.summary_images, csrc/stats.hip): pmd_pixel_stats_accumulate through the C ABI
against NumPy (exactly for integer data, within the forward bound for float data), its state carried over calls, its
bitwise independence of which state it forms, of D, ldy, the element type and the pixel's position, NaN input and bad
arguments; end to end the extrema of every kind against the exported movie bit for bit, the moments against float64
NumPy within a derived bound, the peak-to-noise ratio, invariance over batch sizes, sources, kinds, stats and device
residency, a denoised-only call that reads no movie, and a long uint16 movie summarised in one read with bounded device
memory."""
import numpy as np
import pytest

import localmd_amd
from localmd_amd import decomposition as Dm
from localmd_amd import maps as MP
from localmd_amd import summary as SM
from localmd_amd._lib import PMDLibraryError, ptr
from localmd_amd._minitiff import write_tiff
from localmd_amd.dataset import TiffArray, lazy_data_loader
from localmd_amd.pmdarray import load_npz, save_npz
from tests.consumer_fuzz import check_moments as _check_moments, check_pnr, exported as _exported, extrema_equal_export
from tests.consumer_fuzz import kinds64 as _kinds64, moment_bounds as _moment_bounds  # noqa: F401
from tests.test_gpu_maps import _CountingU16, _decompose, _den64, _int_movie, _long_pmd
from tests.test_summary_host import emulate_bins
from tests.util import degenerate_pmds

pytestmark = pytest.mark.gpu
Dm.QUIET = True
T, D1, D2 = 2500, 40, 44
D = D1 * D2
ALL = ("denoised", "raw", "residual")
U24 = 2.0 ** -24
GAMMA = 1032 * U24
_ELEM = {"float32": 0, "uint16": 1, "int16": 2}
_FILL = {"float32": np.nan, "uint16": 65535, "int16": -32768}      # paddings of Y: they would show up
DS = (1147, 1760)            # 31 x 37 (odd: scalar rows, a ragged last lane) and 40 x 44
NS = (1, 7, 64, 1000, 1024)
BINS = (1, 2, 8, 1024)
_MOMENTS = ("mean", "std", "skewness", "kurtosis")


# ---- the kernel through the C ABI ----------------------------------------------------------------------------------
def _dev(ctx, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _padded(a, ld, src):
    out = np.full((a.shape[0], ld), _FILL[src], dtype=src)
    out[:, :a.shape[1]] = a
    return out


def _fresh(Dn):
    ext = np.empty((2, Dn), np.float32)
    ext[0], ext[1] = np.inf, -np.inf
    return ext, np.full((2, Dn), -1, np.int32), np.zeros((4, Dn), np.float64)


def _stats(ctx, yd, src, ldy, n, Dn, f0, bin, centre, *, form=("ext", "arg", "mom"), state=None):
    """One pmd_pixel_stats_accumulate call on the first n rows of the device batch yd (rows of ldy elements of type
    ``src``) from ``state`` = (ext, arg, mom) (fresh when None).  Returns (ext, arg, mom) as NumPy, None where not formed."""
    s = _fresh(Dn) if state is None else state
    d = [_dev(ctx, a) if k in form else None for k, a in zip(("ext", "arg", "mom"), s)]
    ctx.call("pmd_pixel_stats_accumulate", ptr(yd), _ELEM[src], ldy, n, Dn, f0, bin,
             ptr(None if centre is None else _dev(ctx, np.asarray(centre, np.float32))), ptr(d[0]), ptr(d[1]), ptr(d[2]))
    ctx.sync()
    return tuple(None if t is None else t.cpu().numpy() for t in d)


def _binned_reference(y32, bin, f0):
    """(min, max, argmin, argmax) of the binned series of the (n, N) block: the values of emulate_bins, which for integer
    data are the float64 bin means rounded once (test_summary_host), first occurrences, frame numbers from f0."""
    starts, v = emulate_bins(y32, bin)
    return v.min(axis=0), v.max(axis=0), (f0 + starts[v.argmin(axis=0)]).astype(np.int32), \
        (f0 + starts[v.argmax(axis=0)]).astype(np.int32)


def test_kernel_exact_for_integer_data_every_container_length_bin_and_offset(gpu_ctx):
    """Values 0..6 about the centre 3: ties everywhere, every sum below 2^24 (sum z^4 <= 81 * 1024), so the extrema of the
    binned series, the first frames that attain them and the four power sums are those of NumPy exactly, for every
    container with identical bits."""
    rng = np.random.default_rng(1)
    for Dn in DS:
        Y = rng.integers(0, 7, (1024, Dn))
        centre = np.full(Dn, 3.0, np.float32)
        Z = Y.astype(np.float64) - 3.0
        for ldy in (Dn, Dn + 3):
            dev = {src: _dev(gpu_ctx, _padded(Y, ldy, src)) for src in _ELEM}
            for n in NS:
                want_mom = np.stack([(Z[:n] ** p).sum(axis=0) for p in (1, 2, 3, 4)])
                for bin in BINS:
                    for f0 in (0, 2048):
                        lo, hi, alo, ahi = _binned_reference(Y[:n].astype(np.float32), bin, f0)
                        first = None
                        for src in _ELEM:
                            ext, arg, mom = _stats(gpu_ctx, dev[src], src, ldy, n, Dn, f0, bin, centre)
                            key = (Dn, ldy, n, bin, f0, src)
                            assert np.array_equal(ext[0], lo) and np.array_equal(ext[1], hi), key
                            assert np.array_equal(arg[0], alo) and np.array_equal(arg[1], ahi), key
                            assert np.array_equal(mom, want_mom), key
                            got = ext.tobytes() + arg.tobytes() + mom.tobytes()
                            first = got if first is None else first
                            assert got == first, key


def test_kernel_float_data_within_the_forward_bound(gpu_ctx):
    """fp32 data 900 + 8 N(0, 1) about the centre 900.  Each power sum is within GAMMA sum |z|^p of the float64 sum of the
    same fp32 z (GAMMA = 1032 2^-24: any order of <= 1024 terms plus the three roundings of the powers; the constant of
    maps.GAMMA); a binned extremum is within (bin + 1) 2^-24 mean |y| of the float64 bin mean (at most bin - 1 additions
    and one division, each rounding relative to at most the bin's sum of magnitudes); with bin = 1 it is exact."""
    rng = np.random.default_rng(2)
    assert GAMMA == MP.GAMMA
    worst_m = worst_e = 0.0
    for Dn in DS:
        Y = (900.0 + 8.0 * rng.standard_normal((1024, Dn))).astype(np.float32)
        centre = np.full(Dn, 900.0, np.float32)
        Z = (Y - centre[None, :]).astype(np.float32).astype(np.float64)
        Y64 = Y.astype(np.float64)
        for ldy in (Dn, Dn + 3):
            yd = _dev(gpu_ctx, _padded(Y, ldy, "float32"))
            for n in NS:
                wm = np.stack([(Z[:n] ** p).sum(axis=0) for p in (1, 2, 3, 4)])
                bm = GAMMA * np.stack([(np.abs(Z[:n]) ** p).sum(axis=0) for p in (1, 2, 3, 4)])
                for bin in BINS:
                    f0 = 2048
                    ext, arg, mom = _stats(gpu_ctx, yd, "float32", ldy, n, Dn, f0, bin, centre)
                    key = (Dn, ldy, n, bin)
                    worst_m = max(worst_m, (np.abs(mom - wm) / bm).max())
                    assert np.all(np.abs(mom - wm) <= bm), key
                    starts = np.arange(0, n, bin)
                    means = np.stack([Y64[b:min(n, b + bin)].mean(axis=0) for b in starts])
                    if bin == 1:
                        assert np.array_equal(ext[0], Y[:n].min(axis=0)) and np.array_equal(ext[1], Y[:n].max(axis=0)), key
                        assert np.array_equal(arg[0], f0 + Y[:n].argmin(axis=0)), key
                        assert np.array_equal(arg[1], f0 + Y[:n].argmax(axis=0)), key
                    else:
                        be = (bin + 1) * U24 * np.stack([np.abs(Y64[b:min(n, b + bin)]).mean(axis=0) for b in starts]).max(axis=0)
                        err = np.maximum(np.abs(ext[0] - means.min(axis=0)), np.abs(ext[1] - means.max(axis=0)))
                        worst_e = max(worst_e, (err / be).max())
                        assert np.all(err <= be), key
                        # the frame numbers name bins whose float64 mean is within the bound of the extremum
                        for r, m in ((arg[0], means.min(axis=0)), (arg[1], means.max(axis=0))):
                            assert np.all((r - f0) % bin == 0) and np.all((r >= f0) & (r < f0 + n)), key
                            assert np.all(np.abs(means[(r - f0) // bin, np.arange(Dn)] - m) <= 2 * be), key
                        # and the kernel's own order of summation gives its bits
                        lo, hi, alo, ahi = _binned_reference(Y[:n], bin, f0)
                        assert np.array_equal(ext[0], lo) and np.array_equal(ext[1], hi), key
                        assert np.array_equal(arg[0], alo) and np.array_equal(arg[1], ahi), key
    print("largest error / bound: moments", worst_m, "binned extrema", worst_e)


def test_kernel_state_carries_over_calls_and_keeps_the_first_occurrence(gpu_ctx):
    Dn = 1147
    rng = np.random.default_rng(3)
    Y = rng.integers(10, 20, (2048, Dn))
    Y[100, :] = 50                      # the maximum, in slice 0 of the first call
    Y[500, :] = 50                      # a tie in slice 1 of the same call
    Y[1024 + 50, :] = 50                # and a later tie in the second call
    Y[300, ::2] = 3                     # the minimum of the even pixels in the first call, tied at 900 (another slice)
    Y[900, ::2] = 3
    Y[1024 + 700, :] = 2                # a smaller minimum in the second call: it takes over
    Y[1024 + 800, :] = 2
    centre = np.full(Dn, 15.0, np.float32)
    for src in ("uint16", "float32"):
        a = _dev(gpu_ctx, Y[:1024].astype(src))
        b = _dev(gpu_ctx, Y[1024:].astype(src))
        s1 = _stats(gpu_ctx, a, src, Dn, 1024, Dn, 0, 1, centre)
        assert np.all(s1[1][1] == 100) and np.all(s1[1][0][::2] == 300) and np.all(s1[0][0][::2] == 3)
        assert np.array_equal(s1[1][0][1::2], Y[:1024, 1::2].argmin(axis=0))
        s2 = _stats(gpu_ctx, b, src, Dn, 1024, Dn, 1024, 1, centre, state=s1)
        assert np.all(s2[0][1] == 50) and np.all(s2[1][1] == 100)             # the first occurrence keeps arg
        assert np.all(s2[0][0] == 2) and np.all(s2[1][0] == 1024 + 700)
        Z = Y.astype(np.float64) - 15.0
        assert np.array_equal(s2[2], np.stack([(Z ** p).sum(axis=0) for p in (1, 2, 3, 4)]))
        # the second block alone, and a bin that pairs the tied frames with their neighbours
        alone = _stats(gpu_ctx, b, src, Dn, 1024, Dn, 1024, 1, centre)
        assert np.all(alone[1][1] == 1024 + 50)
        lo, hi, alo, ahi = _binned_reference(Y.astype(np.float32)[:1024], 2, 0)
        t1 = _stats(gpu_ctx, a, src, Dn, 1024, Dn, 0, 2, centre)
        assert np.array_equal(t1[0][1], hi) and np.array_equal(t1[1][1], ahi) and np.array_equal(t1[1][0], alo)
        t2 = _stats(gpu_ctx, b, src, Dn, 1024, Dn, 1024, 2, centre, state=t1)
        lo2, hi2, alo2, ahi2 = _binned_reference(Y.astype(np.float32)[1024:], 2, 1024)
        assert np.array_equal(t2[0][1], np.maximum(hi, hi2)) and np.array_equal(t2[1][1], np.where(hi2 > hi, ahi2, ahi))
        assert np.array_equal(t2[0][0], np.minimum(lo, lo2)) and np.array_equal(t2[1][0], np.where(lo2 < lo, alo2, alo))


def test_kernel_bits_do_not_depend_on_what_it_forms_nor_on_the_embedding(gpu_ctx):
    rng = np.random.default_rng(4)
    Dn, n, f0 = 1147, 1000, 2048
    Y = (900.0 + 8.0 * rng.standard_normal((1024, Dn))).astype(np.float32)
    centre = (900.0 + rng.standard_normal(Dn)).astype(np.float32)
    yd = _dev(gpu_ctx, Y)
    for bin in (1, 8, 512):
        ext, arg, mom = _stats(gpu_ctx, yd, "float32", Dn, n, Dn, f0, bin, centre)
        # split state
        e1, a1, m1 = _stats(gpu_ctx, yd, "float32", Dn, n, Dn, f0, bin, centre, form=("ext", "arg"))
        assert m1 is None and e1.tobytes() == ext.tobytes() and a1.tobytes() == arg.tobytes()
        e2, a2, m2 = _stats(gpu_ctx, yd, "float32", Dn, n, Dn, f0, bin, centre, form=("mom",))
        assert e2 is None and a2 is None and m2.tobytes() == mom.tobytes()
        e3, a3, m3 = _stats(gpu_ctx, yd, "float32", Dn, n, Dn, f0, bin, centre, form=("ext", "mom"))
        assert a3 is None and e3.tobytes() == ext.tobytes() and m3.tobytes() == mom.tobytes()
        e4, _, _ = _stats(gpu_ctx, yd, "float32", Dn, n, Dn, f0, bin, None, form=("ext",))
        assert e4.tobytes() == ext.tobytes()
        # the same columns inside a wider batch: other D, other ldy (aligned rows and rows that are not), shifted position
        for Dw, ldw, off in ((1760, 1760, 5), (1760, 1763, 256), (1300, 1304, 153)):
            W = rng.standard_normal((1024, ldw)).astype(np.float32)
            W[:, Dw:] = np.nan
            W[:, off:off + Dn] = Y
            cw = np.zeros(Dw, np.float32)
            cw[off:off + Dn] = centre
            ew, aw, mw = _stats(gpu_ctx, _dev(gpu_ctx, W), "float32", ldw, n, Dw, f0, bin, cw)
            key = (bin, Dw, ldw, off)
            assert np.ascontiguousarray(ew[:, off:off + Dn]).tobytes() == ext.tobytes(), key
            assert np.ascontiguousarray(aw[:, off:off + Dn]).tobytes() == arg.tobytes(), key
            assert np.ascontiguousarray(mw[:, off:off + Dn]).tobytes() == mom.tobytes(), key


def test_kernel_nan_input(gpu_ctx):
    rng = np.random.default_rng(5)
    Dn, n, px = 1147, 300, 10
    Y = (900.0 + 8.0 * rng.standard_normal((n, Dn))).astype(np.float32)
    Yn = Y.copy()
    Yn[3, px] = np.nan
    rest = np.delete(np.arange(n), 3)
    for bin in (1, 2):
        clean = _stats(gpu_ctx, _dev(gpu_ctx, Y), "float32", Dn, n, Dn, 0, bin, None)
        ext, arg, mom = _stats(gpu_ctx, _dev(gpu_ctx, Yn), "float32", Dn, n, Dn, 0, bin, None)
        if bin == 1:        # the NaN frame is ignored: the extrema of the other frames
            assert ext[0][px] == Y[rest, px].min() and ext[1][px] == Y[rest, px].max()
            assert arg[0][px] == rest[Y[rest, px].argmin()] and arg[1][px] == rest[Y[rest, px].argmax()]
        else:               # its bin (frames 2, 3) is ignored
            starts, v = emulate_bins(Y, 2)
            v = np.delete(v[:, px], 1)
            assert ext[0][px] == v.min() and ext[1][px] == v.max() and arg[0][px] != 2 and arg[1][px] != 2
        assert np.all(np.isfinite(ext)) and np.all(np.isnan(mom[:, px]))
        keep = np.arange(Dn) != px
        for got, want in zip((ext, arg, mom), clean):
            assert np.array_equal(got[:, keep], want[:, keep])


def test_kernel_rejects_bad_arguments(gpu_ctx):
    import torch

    Dn = 35
    y = torch.zeros((8, 40), dtype=torch.float32, device=gpu_ctx.device)
    state = [_dev(gpu_ctx, a) for a in _fresh(Dn)]
    state[2] += 7.0
    before = [t.clone() for t in state]
    centre = torch.zeros(Dn, dtype=torch.float32, device=gpu_ctx.device)
    names = ["Y", "elem", "ldy", "n", "D", "f0", "bin", "centre", "ext", "arg", "mom"]
    good = [ptr(y), 0, 40, 4, Dn, 0, 1, ptr(centre), ptr(state[0]), ptr(state[1]), ptr(state[2])]

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        with pytest.raises(PMDLibraryError, match=r"failed \(-2\)"):      # PMD_ERR_ARG
            gpu_ctx.call("pmd_pixel_stats_accumulate", *a)

    bad(n=0)
    bad(n=-1)
    bad(n=1025)
    bad(bin=0)
    bad(bin=3)
    bad(bin=2048)
    bad(bin=-4)
    bad(bin=8, f0=4)                    # f0 is not a multiple of bin
    bad(f0=-1)
    bad(f0=2 ** 31 - 4)                 # f0 + n reaches 2^31
    bad(ext=None, arg=None, mom=None)
    bad(ext=None)                       # arg without ext
    bad(elem=7)
    bad(elem=-1)
    bad(ldy=Dn - 1)
    bad(D=0, ldy=0)
    bad(Y=None)
    gpu_ctx.sync()
    for t, b in zip(state, before):
        assert torch.equal(t, b)
    gpu_ctx.call("pmd_pixel_stats_accumulate", *good)                     # and the good call is one
    gpu_ctx.sync()
    assert float(state[0][0].max()) == 0.0 and int(state[1].max()) == 0


# ---- end to end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(gpu_ctx):
    mov = _int_movie(4)
    return mov, {o: _decompose(gpu_ctx, mov, o) for o in ("F", "C")}


def _check_extrema_against_export(ctx, pmd, mov):
    panels = _exported(ctx, pmd, mov)
    assert np.array_equal(panels["raw"], mov.reshape(T, D))
    s = localmd_amd.summary_images(pmd, mov, kinds=ALL, stats=("min", "max", "argmin", "argmax"), frame_batch_size=1024,
                                   ctx=ctx)
    assert s.stats == ("min", "max", "argmin", "argmax") and s.temporal_bin == 1
    for kind in ALL:
        assert sorted(getattr(s, kind)) == ["argmax", "argmin", "max", "min"]
    extrema_equal_export({k: getattr(s, k) for k in ALL}, panels, D1, D2)
    assert np.array_equal(s.raw["max"], mov.max(axis=0)) and np.array_equal(s.raw["argmax"], mov.argmax(axis=0))
    return s


@pytest.mark.parametrize("order", ["F", "C"])
def test_extrema_are_those_of_the_exported_movie_bit_for_bit(gpu_ctx, case, order):
    mov, pmds = case
    _check_extrema_against_export(gpu_ctx, pmds[order], mov)
    # bins of 8 frames: the float64 bin means of the integer movie rounded to fp32, the short last bin included
    assert T == 312 * 8 + 4
    Y64 = mov.reshape(T, D).astype(np.float64)
    means = np.stack([Y64[b:b + 8].mean(axis=0) for b in range(0, T, 8)]).astype(np.float32)
    assert len(means) == 313
    b = localmd_amd.summary_images(pmds[order], mov.astype(np.uint16), kinds="raw", stats=("min", "max", "argmin", "argmax"),
                                   temporal_bin=8, ctx=gpu_ctx)
    assert b.temporal_bin == 8 and b.denoised is None and b.residual is None
    assert np.array_equal(b.raw["min"].reshape(-1), means.min(axis=0))
    assert np.array_equal(b.raw["max"].reshape(-1), means.max(axis=0))
    assert np.array_equal(b.raw["argmin"].reshape(-1), 8 * means.argmin(axis=0))
    assert np.array_equal(b.raw["argmax"].reshape(-1), 8 * means.argmax(axis=0))
    # the last bin can win: a movie whose last four frames hold the maximum
    late = mov.copy()
    late[T - 4:] += 4000.0
    b = localmd_amd.summary_images(pmds[order], late, kinds="raw", stats=("max", "argmax"), temporal_bin=8, ctx=gpu_ctx)
    assert np.all(b.raw["argmax"] == T - 4)
    assert np.array_equal(b.raw["max"].reshape(-1), late.reshape(T, D)[T - 4:].astype(np.float64).mean(axis=0).astype(np.float32))


def test_background_rank_zero(gpu_ctx, case):
    mov = case[0]
    pmd = _decompose(gpu_ctx, mov, "F", background_rank=0)
    _check_extrema_against_export(gpu_ctx, pmd, mov)
    s = localmd_amd.summary_images(pmd, mov, kinds=ALL, stats=_MOMENTS, ctx=gpu_ctx)
    _check_moments(s, pmd, mov)


@pytest.mark.parametrize("which", ["no_columns", "rank_zero"])
def test_decomposition_without_columns_or_rank(gpu_ctx, case, which):
    """The denoised movie is the mean image: extrema against the export as for any decomposition, and a constant pixel's
    moments."""
    mov, pmds = case
    pmd = degenerate_pmds(pmds["C"])[which]
    mean32 = np.asarray(pmd.mean_img, np.float32)
    s = _check_extrema_against_export(gpu_ctx, pmd, mov)
    assert np.array_equal(s.denoised["min"], mean32) and np.array_equal(s.denoised["max"], mean32)
    assert not s.denoised["argmin"].any() and not s.denoised["argmax"].any()
    m = localmd_amd.summary_images(pmd, mov, kinds="denoised", stats=("mean", "std"), ctx=gpu_ctx).denoised
    assert np.array_equal(m["mean"], mean32) and not m["std"].any()


@pytest.mark.parametrize("order", ["F", "C"])
def test_moments_against_fp64_and_pnr(gpu_ctx, case, order):
    mov, pmds = case
    pmd = pmds[order]
    s = localmd_amd.summary_images(pmd, mov, kinds=ALL, stats=_MOMENTS + ("max", "pnr"), frame_batch_size=2048, ctx=gpu_ctx)
    _check_moments(s, pmd, mov)
    # pnr: (max - mean) / noise in float64 from the returned float32 max and the float64 mean, rounded once
    check_pnr(s, pmd, mov)
    import copy

    # where the noise image is unusable the ratio is 0
    import copy

    broken = copy.copy(pmd)
    broken.var_img = np.array(pmd.var_img, copy=True)
    broken.var_img[3, 4], broken.var_img[5, 6], broken.var_img[7, 8] = 0.0, np.nan, np.inf
    p = localmd_amd.summary_images(broken, mov, kinds="raw", stats="pnr", ctx=gpu_ctx).raw["pnr"]
    assert p[3, 4] == 0 and p[5, 6] == 0 and p[7, 8] == 0
    keep = np.ones((D1, D2), bool)
    keep[[3, 5, 7], [4, 6, 8]] = False
    assert np.array_equal(p[keep], s.raw["pnr"][keep])


# ---- invariance ----------------------------------------------------------------------------------------------------
def _bytes(s, kinds=ALL, stats=SM.STATS):
    return b"".join(getattr(s, k)[st].tobytes() for k in kinds for st in stats)


def test_batch_source_kind_stat_and_residency_invariance(gpu_ctx, case, tmp_path):
    import torch

    mov, pmds = case
    pmd = pmds["F"]
    kw = dict(kinds=ALL, stats=SM.STATS, temporal_bin=8, ctx=gpu_ctx)
    ref = localmd_amd.summary_images(pmd, mov, frame_batch_size=1024, **kw)
    want = _bytes(ref)
    assert repr(ref) == "Summary(denoised, raw, residual; {}; temporal_bin=8)".format(", ".join(SM.STATS))
    for fbs in (100, 1024, 10000):
        assert _bytes(localmd_amd.summary_images(pmd, mov, frame_batch_size=fbs, **kw)) == want, fbs
    u16 = mov.astype(np.uint16)
    mm = np.lib.format.open_memmap(str(tmp_path / "m.npy"), mode="w+", dtype=np.uint16, shape=mov.shape)
    mm[:] = u16
    path = str(tmp_path / "movie.tif")
    write_tiff(path, u16)
    sources = {"numpy_u16": u16, "memmap": mm, "cpu_tensor": torch.from_numpy(mov), "tiff": TiffArray(path),
               "device_tensor": torch.from_numpy(mov).to(gpu_ctx.device),
               "device_i16": torch.from_numpy(mov.astype(np.int16)).to(gpu_ctx.device)}
    for name, src in sources.items():
        assert _bytes(localmd_amd.summary_images(pmd, src, frame_batch_size=2048, **kw)) == want, name
    # kinds in another order, and one at a time
    got = localmd_amd.summary_images(pmd, mov, kinds=("residual", "raw", "denoised"), stats=SM.STATS, temporal_bin=8,
                                     ctx=gpu_ctx)
    assert _bytes(got) == want
    for kind in ALL:
        one = localmd_amd.summary_images(pmd, u16, kinds=kind, stats=SM.STATS, temporal_bin=8, frame_batch_size=1024,
                                         ctx=gpu_ctx)
        assert [k for k in ALL if getattr(one, k) is not None] == [kind]
        assert _bytes(one, (kind,)) == _bytes(ref, (kind,)), kind
    # stats one at a time against all at once
    for stat in SM.STATS:
        one = localmd_amd.summary_images(pmd, mov, kinds=ALL, stats=stat, temporal_bin=8, ctx=gpu_ctx)
        assert one.stats == (stat,) and sorted(one.raw) == [stat]
        assert _bytes(one, ALL, (stat,)) == _bytes(ref, ALL, (stat,)), stat
    # device-resident factors
    pmd.to_device(ctx=gpu_ctx)
    try:
        got = pmd.summary(mov, kinds=ALL, stats=SM.STATS, temporal_bin=8)
    finally:
        pmd.to_host()
    assert _bytes(got) == want
    # a decomposition read back from disk, and the method against the function
    npz = str(tmp_path / "pmd.npz")
    save_npz(npz, pmd)
    assert _bytes(localmd_amd.summary_images(load_npz(npz), mov, **kw)) == want
    assert _bytes(pmd.summary(mov, **kw)) == want


class _Untouchable(lazy_data_loader):
    dtype = property(lambda self: np.float32)
    shape = property(lambda self: (T, D1, D2))

    def _compute_at_indices(self, indices):
        raise AssertionError("the movie was read")


def test_denoised_only_reads_no_movie(gpu_ctx, case):
    mov, pmds = case
    pmd = pmds["C"]
    a = localmd_amd.summary_images(pmd, ctx=gpu_ctx)                    # kinds "denoised", stats mean / std / max
    b = localmd_amd.summary_images(pmd, _Untouchable(), kinds=("denoised",), ctx=gpu_ctx)
    c = localmd_amd.summary_images(pmd, mov, kinds=ALL, ctx=gpu_ctx)
    assert a.stats == ("mean", "std", "max") and a.raw is None and a.residual is None and b.raw is None
    assert _bytes(a, ("denoised",), a.stats) == _bytes(b, ("denoised",), a.stats) == _bytes(c, ("denoised",), a.stats)


# ---- a long movie --------------------------------------------------------------------------------------------------
def test_long_movie_read_once_bounded_memory(gpu_ctx):
    import torch

    d1 = d2 = 64
    px = [(0, 0), (31, 40), (63, 63)]
    peaks = {}
    for n in (8000, 40000):
        src = _CountingU16(n, d1, d2)
        pmd = _long_pmd(n, d1, d2)
        gpu_ctx.release_workspace()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        s = localmd_amd.summary_images(pmd, src, kinds=ALL, stats=SM.STATS, frame_batch_size=4096, ctx=gpu_ctx)
        peaks[n] = torch.cuda.max_memory_allocated() - base
        assert np.all(src.count == 1), np.unique(src.count)
        t = np.arange(n)
        for i, j in px:
            y = src.noise[(t * 7919) % 64, i, j].astype(np.float32) + (t % 1000).astype(np.float32)
            assert s.raw["max"][i, j] == y.max() and s.raw["argmax"][i, j] == y.argmax(), (n, i, j)
            assert s.raw["min"][i, j] == y.min() and s.raw["argmin"][i, j] == y.argmin(), (n, i, j)
        for kind in ALL:
            assert all(np.all(np.isfinite(a)) for a in getattr(s, kind).values()), kind
    print("peak device bytes", peaks)
    assert peaks[40000] <= peaks[8000], peaks
