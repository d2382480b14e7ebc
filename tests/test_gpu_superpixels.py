"""Superpixels on the GPU (localmd_amd.superpixels, csrc/superpixel.hip): pmd_threshold_moments_accumulate through the C ABI
against NumPy (exactly for integer data, bit for bit against the sequential fp64 chains of tests/superpixel_ref.py for
float data), its independence of the split into calls, of ldy, the element type and the pixel's position, special values
and bad arguments; pmd_grid_components exactly against scipy's connected components on paths, spirals, diagonals, the
crossing pair and random graphs around the percolation threshold; superpixels end to end against superpixels_ref on the
exported movie, its invariances, the number of reads of the movie, bounded device memory, and planted cells through to
demix."""
import importlib

import numpy as np
import pytest
import scipy.sparse

import localmd_amd
from localmd_amd._lib import ptr
from localmd_amd._minitiff import write_tiff
from localmd_amd.dataset import TiffArray, lazy_data_loader
from localmd_amd.pmdarray import PMDArray
from tests import superpixel_ref as SR
from tests.consumer_fuzz import superpixels_equal_reference as _check_against_reference
from tests.test_gpu_demix import _pmd
from tests.test_gpu_maps import _CountingU16, _long_pmd
from tests.test_traces_host import _disc

pytestmark = pytest.mark.gpu
SP = importlib.import_module("localmd_amd.superpixels")
ERR_ARG, ERR_WORKSPACE = -2, -3
_ELEM = {"float32": 0, "uint16": 1, "int16": 2}
_FILL = {"float32": np.nan, "uint16": 65535, "int16": -32768}      # paddings of Y: they would show up
SHAPES = ((1, 1), (1, 70), (70, 1), (31, 37), (40, 44), (65, 130))   # one wave owns 62 columns, a workgroup 8 rows
NS = (1, 7, 64, 1000, 1024)


def _dev(ctx, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _padded(a, ld, src):
    """(n, d1, d2) -> (n, ld) of dtype ``src`` with poisoned padding."""
    n = a.shape[0]
    out = np.full((n, ld), _FILL[src], dtype=src)
    out[:, :a[0].size] = a.reshape(n, -1)
    return out


def _moments(ctx, yd, src, ldy, n, d1, d2, thr, start=None, f0=0):
    """One pmd_threshold_moments_accumulate call on the n frames from row f0 of the device batch yd; returns mom."""
    import ctypes as C

    mom = _dev(ctx, np.zeros((6, d1 * d2)) if start is None else start)
    at = C.c_void_p(yd.data_ptr() + f0 * ldy * yd.element_size())
    ctx.call("pmd_threshold_moments_accumulate", at, _ELEM[src], ldy, n, d1, d2, ptr(_dev(ctx, np.asarray(thr, np.float32))),
             ptr(mom))
    ctx.sync()
    return mom.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ---- pmd_threshold_moments_accumulate ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_moments_exact_for_integer_data(gpu_ctx, shape):
    """Values 0 .. 6 against thr = 3: y is in 0 .. 3 and every sum an integer below 2^53, so the chains equal NumPy's
    integer sums exactly, for every length, leading dimension and element type, with identical bits across the types."""
    d1, d2 = shape
    D = d1 * d2
    rng = np.random.default_rng(d1 * 1000 + d2)
    Y = rng.integers(0, 7, (1024, d1, d2))
    y = np.maximum(Y - 3, 0)
    nb = [y] + [SR.neighbour(y, di, dj) for di, dj in SR.FORWARD]
    thr = np.full(D, 3.0, np.float32)
    for ldy in (D, D + 3):
        dev = {src: _dev(gpu_ctx, _padded(Y, ldy, src)) for src in _ELEM}
        for n in NS:
            want = np.stack([y[:n].sum(axis=0), (y[:n] * y[:n]).sum(axis=0)] + [(y[:n] * q[:n]).sum(axis=0) for q in nb[1:]])
            want = want.reshape(6, D).astype(np.float64)
            first = None
            for src in _ELEM:
                got = _moments(gpu_ctx, dev[src], src, ldy, n, d1, d2, thr)
                assert np.array_equal(got, want), (shape, ldy, n, src)
                first = got.tobytes() if first is None else first
                assert got.tobytes() == first, (shape, ldy, n, src)


@pytest.fixture(scope="module")
def float_case():
    """{shape: (Y, thr, {n: reference moments})} for float data 100 + 5 N(0, 1) against thresholds around 100."""
    out = {}
    for d1, d2 in ((31, 37), (65, 130)):
        rng = np.random.default_rng(d1)
        Y = (100.0 + 5.0 * rng.standard_normal((1024, d1, d2))).astype(np.float32)
        thr = (100.0 + rng.standard_normal((d1, d2))).astype(np.float32)
        out[d1, d2] = (Y, thr, SR.moments_at(SR.rectified(Y, thr), (7, 1000, 1024)))
    return out


@pytest.mark.parametrize("shape", [(31, 37), (65, 130)])
def test_moments_float_data_bit_for_bit_and_split_over_calls(gpu_ctx, float_case, shape):
    d1, d2 = shape
    D = d1 * d2
    Y, thr, ref = float_case[shape]
    for ldy in (D, D + 3):
        yd = _dev(gpu_ctx, _padded(Y, ldy, "float32"))
        whole = _moments(gpu_ctx, yd, "float32", ldy, 1024, d1, d2, thr)
        assert _same_bits(whole, ref[1024]), (shape, ldy)
        for k in (1000, 7):
            part = _moments(gpu_ctx, yd, "float32", ldy, k, d1, d2, thr)
            assert _same_bits(part, ref[k]), (shape, ldy, k)
            both = _moments(gpu_ctx, yd, "float32", ldy, 1024 - k, d1, d2, thr, start=part, f0=k)
            assert _same_bits(both, whole), (shape, ldy, k)
    # the reference continued from a state is the reference of the whole
    assert _same_bits(SR.moments(SR.rectified(Y[7:], thr), start=ref[7]), ref[1024])


def test_moments_bits_do_not_depend_on_the_position(gpu_ctx, float_case):
    """The 31 x 37 image inside a larger one, away from its last row and column: a pixel whose forward neighbours lie
    inside the small image keeps every bit; S1 and S2 of every pixel do."""
    d1, d2 = 31, 37
    Y, thr, ref = float_case[d1, d2]
    want = ref[1000].reshape(6, d1, d2)
    rng = np.random.default_rng(11)
    for (e1, e2), (oi, oj) in (((50, 100), (3, 5)), ((50, 100), (10, 60)), ((40, 140), (8, 63)), ((33, 40), (1, 2))):
        W = (100.0 + 5.0 * rng.standard_normal((1000, e1, e2))).astype(np.float32)
        tw = (100.0 + rng.standard_normal((e1, e2))).astype(np.float32)
        W[:, oi:oi + d1, oj:oj + d2] = Y[:1000]
        tw[oi:oi + d1, oj:oj + d2] = thr
        got = _moments(gpu_ctx, _dev(gpu_ctx, W.reshape(1000, -1)), "float32", e1 * e2, 1000, e1, e2, tw)
        got = got.reshape(6, e1, e2)[:, oi:oi + d1, oj:oj + d2]
        assert _same_bits(got[:2], want[:2]), (e1, e2, oi, oj)
        assert _same_bits(got[:, :d1 - 1, 1:d2 - 1], want[:, :d1 - 1, 1:d2 - 1]), (e1, e2, oi, oj)


def test_moments_special_values(gpu_ctx):
    d1, d2, n = 9, 70, 40
    D = d1 * d2
    rng = np.random.default_rng(12)
    Y = (100.0 + 5.0 * rng.standard_normal((n, d1, d2))).astype(np.float32)
    thr = np.full((d1, d2), 99.0, np.float32)
    Y[5] = np.nan                       # a NaN frame: y = 0 in that frame, everywhere
    thr[2, 3] = np.nan                  # a NaN threshold: the pixel's y is 0 throughout
    Y[7, 4, 61] = np.inf                # +inf: the sums of the pixel and of its pairs are not finite
    Y[:, 6, 10] = 123.0                 # a constant column (the NaN frame included)
    thr[8, :] = 1e6                     # above every value: the last row is 0
    want = SR.moments(SR.rectified(Y, thr))
    got = _moments(gpu_ctx, _dev(gpu_ctx, Y.reshape(n, -1)), "float32", D, n, d1, d2, thr)
    assert np.array_equal(got, want, equal_nan=True)
    finite = np.isfinite(want)
    assert _same_bits(got[finite], want[finite])
    g = got.reshape(6, d1, d2)
    assert not g[:, 2, 3].any() and not g[:, 8, :].any()
    assert g[0, 6, 10] == n * 24.0 and g[1, 6, 10] == n * 576.0
    assert np.isfinite(g[0, 6, 11]) and g[0, 6, 11] > 0                               # the NaN frame counted 0
    assert np.isinf(g[0, 4, 61]) and np.isinf(g[1, 4, 61]) and not np.isfinite(g[2, 4, 60])
    assert np.all(np.isfinite(g[:, :, :58]))
    rho = SP.finish_correlations(got, n, d1, d2)
    e = SP.edge_bytes(rho, -1.0)
    assert e[4, 61] == 0 and not (e[4, 60] & 1) and not (e[3, 61] & 4) and not (e[3, 62] & 2) and not (e[3, 60] & 8)
    assert np.array_equal(e, SR.edge_byte(SR.finish(want, n, d1, d2), -1.0))


def test_moments_bad_arguments_leave_mom_untouched(gpu_ctx):
    import torch

    d1, d2 = 5, 7
    y = torch.zeros((8, 40), dtype=torch.float32, device=gpu_ctx.device)
    thr = torch.zeros(35, dtype=torch.float32, device=gpu_ctx.device)
    mom = torch.full((6, 35), 7.0, dtype=torch.float64, device=gpu_ctx.device)
    names = ["Y", "elem", "ldy", "n", "d1", "d2", "thr", "mom"]
    good = [ptr(y), 0, 40, 4, d1, d2, ptr(thr), ptr(mom)]
    lib, h = gpu_ctx.lib, gpu_ctx.handle

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        assert lib.pmd_threshold_moments_accumulate(h, *a) == ERR_ARG, kw

    bad(n=0), bad(n=-3), bad(d1=0), bad(d2=0), bad(d1=-1), bad(ldy=34), bad(elem=3), bad(elem=-1)
    bad(Y=None), bad(thr=None), bad(mom=None)
    gpu_ctx.sync()
    assert torch.equal(mom, torch.full_like(mom, 7.0))
    y += 2.0
    assert lib.pmd_threshold_moments_accumulate(h, *good) == 0
    gpu_ctx.sync()
    m = mom.cpu().numpy().reshape(6, d1, d2)
    assert np.all(m[0] == 7.0 + 8.0) and np.all(m[1] == 7.0 + 16.0) and m[2, 0, 0] == 23.0 and m[2, 0, 6] == 7.0


# ---- pmd_grid_components -------------------------------------------------------------------------------------------
CC_SHAPES = SHAPES + ((129, 130),)      # a tile is 16 x 64: the last spans several tiles in both directions


def _components(ctx, edges, bufs=None):
    import torch

    d1, d2 = edges.shape
    nws = int(ctx.lib.pmd_grid_components_workspace_bytes(d1, d2))
    assert nws > 0
    if bufs is None:
        bufs = (torch.full((d1, d2), -7, dtype=torch.int32, device=ctx.device),
                torch.full((nws,), 255, dtype=torch.uint8, device=ctx.device))
    ctx.call("pmd_grid_components", d1, d2, ptr(_dev(ctx, edges)), ptr(bufs[0]), ptr(bufs[1]), nws)
    return bufs[0].cpu().numpy(), bufs


def _path_edges(path, d1, d2):
    """The edge bytes of a path of 4-connected pixels."""
    e = np.zeros((d1, d2), np.uint8)
    for (i, j), (p, q) in zip(path[:-1], path[1:]):
        assert abs(i - p) + abs(j - q) == 1
        if i == p:
            e[i, min(j, q)] |= 1        # E of the left pixel
        else:
            e[min(i, p), j] |= 4        # S of the upper pixel
    return e


def _serpentine(d1, d2):
    return [(i, j if i % 2 == 0 else d2 - 1 - j) for i in range(d1) for j in range(d2)]


def _spiral(d1, d2):
    """Inwards from (0, 0), leaving a free ring between the turns: a path of about D / 2 pixels and free pixels."""
    free = np.ones((d1, d2), bool)
    path, (i, j), k = [(0, 0)], (0, 0), 0
    free[0, 0] = False
    steps = ((0, 1), (1, 0), (0, -1), (-1, 0))

    def ok(p, q, frm):
        if not (0 <= p < d1 and 0 <= q < d2 and free[p, q]):
            return False
        for a, b in steps:              # touches no earlier part of the path but the pixel it comes from
            if (p + a, q + b) != frm and 0 <= p + a < d1 and 0 <= q + b < d2 and not free[p + a, q + b]:
                return False
        return True

    turns = 0
    while turns < 2:
        di, dj = steps[k]
        if ok(i + di, j + dj, (i, j)):
            i, j = i + di, j + dj
            free[i, j] = False
            path.append((i, j))
            turns = 0
        else:
            k, turns = (k + 1) % 4, turns + 1
    return path


def _random_edges(d1, d2, density, seed, bits=(0, 1, 2, 3)):
    rng = np.random.default_rng(seed)
    e = np.zeros((d1, d2), np.uint8)
    for b in bits:
        e |= (rng.random((d1, d2)) < density).astype(np.uint8) << np.uint8(b)
    return e


@pytest.mark.parametrize("shape", CC_SHAPES)
def test_components_exact(gpu_ctx, shape):
    d1, d2 = shape
    D = d1 * d2
    idx = np.arange(D, dtype=np.int32).reshape(d1, d2)
    cases = {"none": np.zeros((d1, d2), np.uint8), "all": np.full((d1, d2), 15, np.uint8),
             "all, high bits set": np.full((d1, d2), 255, np.uint8),
             "serpentine": _path_edges(_serpentine(d1, d2), d1, d2), "spiral": _path_edges(_spiral(d1, d2), d1, d2),
             "diagonals": _random_edges(d1, d2, 0.5, 1, bits=(1, 3)), "SE only": np.full((d1, d2), 8, np.uint8),
             "SW only": np.full((d1, d2), 2, np.uint8)}
    for density in (0.05, 0.2, 0.35, 0.6):
        cases["random %.2f" % density] = _random_edges(d1, d2, density, int(100 * density) + d1)
    bufs = None
    for name, edges in cases.items():
        want = SR.components(edges & 15, d1, d2)
        got, bufs = _components(gpu_ctx, edges, bufs)           # every call into the same buffers
        assert got.dtype == np.int32 and np.array_equal(got, want), (shape, name)
        again, _ = _components(gpu_ctx, edges, bufs)
        assert np.array_equal(again, want), (shape, name, "second call")
    assert np.array_equal(SR.components(cases["none"], d1, d2), idx)
    assert not SR.components(cases["all"], d1, d2).any() and not SR.components(cases["serpentine"], d1, d2).any()
    if min(d1, d2) > 4:
        sp = SR.components(cases["spiral"], d1, d2)
        assert (sp == 0).sum() == len(_spiral(d1, d2)) > D // 3 and len(np.unique(sp)) > 1


def test_components_crossing_diagonals_stay_apart(gpu_ctx):
    """(i, j) - (i + 1, j + 1) by SE and (i, j + 1) - (i + 1, j) by SW cross without meeting: two components, inside a
    tile, across a tile's corner (rows 15 | 16, columns 63 | 64) and at the image's last corner."""
    for d1, d2, i, j in ((2, 2, 0, 0), (40, 130, 3, 5), (40, 130, 15, 63), (40, 130, 15, 10), (40, 130, 7, 63),
                         (40, 130, 38, 128)):
        e = np.zeros((d1, d2), np.uint8)
        e[i, j], e[i, j + 1] = 8, 2
        got, _ = _components(gpu_ctx, e)
        want = np.arange(d1 * d2, dtype=np.int32).reshape(d1, d2)
        want[i + 1, j + 1], want[i + 1, j] = want[i, j], want[i, j + 1]
        assert np.array_equal(got, want), (d1, d2, i, j)
        assert np.array_equal(SR.components(e, d1, d2), want)


def test_components_bad_arguments(gpu_ctx):
    import torch

    lib, h = gpu_ctx.lib, gpu_ctx.handle
    e = torch.zeros((4, 6), dtype=torch.uint8, device=gpu_ctx.device)
    lab = torch.full((4, 6), -7, dtype=torch.int32, device=gpu_ctx.device)
    nws = int(lib.pmd_grid_components_workspace_bytes(4, 6))
    ws = torch.zeros(nws, dtype=torch.uint8, device=gpu_ctx.device)
    assert lib.pmd_grid_components_workspace_bytes(0, 6) == 0 and lib.pmd_grid_components_workspace_bytes(4, -1) == 0
    assert lib.pmd_grid_components(h, 0, 6, ptr(e), ptr(lab), ptr(ws), nws) == ERR_ARG
    assert lib.pmd_grid_components(h, 4, 0, ptr(e), ptr(lab), ptr(ws), nws) == ERR_ARG
    assert lib.pmd_grid_components(h, -4, 6, ptr(e), ptr(lab), ptr(ws), nws) == ERR_ARG
    assert lib.pmd_grid_components(h, 1 << 16, 1 << 15, ptr(e), ptr(lab), ptr(ws), nws) == ERR_ARG      # D = 2^31
    assert lib.pmd_grid_components(h, 4, 6, None, ptr(lab), ptr(ws), nws) == ERR_ARG
    assert lib.pmd_grid_components(h, 4, 6, ptr(e), None, ptr(ws), nws) == ERR_ARG
    assert lib.pmd_grid_components(h, 4, 6, ptr(e), ptr(lab), None, nws) == ERR_ARG
    assert lib.pmd_grid_components(h, 4, 6, ptr(e), ptr(lab), ptr(ws), nws - 1) == ERR_WORKSPACE
    gpu_ctx.sync()
    assert int(lab.min()) == -7 and int(lab.max()) == -7
    assert lib.pmd_grid_components(h, 4, 6, ptr(e), ptr(lab), ptr(ws), nws) == 0
    assert np.array_equal(lab.cpu().numpy().reshape(-1), np.arange(24))


# ---- superpixels end to end ----------------------------------------------------------------------------------------
T, D1, D2 = 300, 24, 20


def _exported(ctx, pmd):
    out = np.empty(tuple(pmd.shape), np.float32)
    localmd_amd.export_movie(pmd, out, panels="denoised", dtype="float32", ctx=ctx)
    return out


def _raw_movie(X, seed=21, w=7):
    """An integer-valued movie (exact in uint16) of the shape of X: sums of white noise over w x w windows, so neighbouring
    pixels correlate at about (w - 1) / w, plus independent noise whose level differs from pixel to pixel, so the
    correlations spread from about 0.2 to 0.9."""
    rng = np.random.default_rng(seed)
    n, d1, d2 = X.shape
    a = rng.standard_normal((n, d1 + w - 1, d2 + w - 1))
    box = sum(a[:, i:i + d1, j:j + d2] for i in range(w) for j in range(w))
    own = rng.uniform(0.0, 2.0, (d1, d2)) ** 2 * rng.standard_normal((n, d1, d2))
    return np.rint(1000.0 + 30.0 * (box / w + own)).astype(np.float32)


@pytest.fixture(scope="module")
def e2e(gpu_ctx):
    pmd = _pmd("F")
    X = _exported(gpu_ctx, pmd)
    return pmd, X, _raw_movie(X)


@pytest.mark.parametrize("kind", ["denoised", "raw"])
def test_superpixels_equal_the_reference_on_the_exported_movie(gpu_ctx, e2e, kind):
    pmd, X, raw = e2e
    movie = {"denoised": X, "raw": raw}[kind]
    found = 0
    for th in (2.0, 0.0):
        for cut_off in (0.9, 0.5):
            ref = SR.superpixels_ref(movie, th=th, cut_off=cut_off, min_size=2)
            sp = localmd_amd.superpixels(pmd, raw if kind == "raw" else None, kind=kind, th=th, cut_off=cut_off, min_size=2,
                                         ctx=gpu_ctx)
            assert (sp.kind, sp.th, sp.cut_off, sp.min_size, sp.max_size) == (kind, th, cut_off, 2, None)
            _check_against_reference(sp, ref, cut_off, (kind, th, cut_off))
            found += len(sp.sizes)
    assert found > 0
    # the size filter, and the labels as ROIs of demix
    ref = SR.superpixels_ref(movie, th=0.0, cut_off=0.5, min_size=3, max_size=40)
    sp = pmd.superpixels(raw, kind=kind, th=0.0, cut_off=0.5, min_size=3, max_size=40, ctx=gpu_ctx)
    _check_against_reference(sp, ref, 0.5, (kind, "filtered"))
    if len(sp.sizes):
        dm = pmd.demix(sp.labels, outer_iters=1, sweeps=1, ctx=gpu_ctx)
        assert dm.traces.shape == (len(sp.sizes), T) and np.array_equal(dm.labels, np.arange(1, len(sp.sizes) + 1))


def _bytes(sp):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (sp.labels, sp.sizes, sp.correlation, sp.threshold, sp.edges)) \
        + str(sp.n_components).encode()


def test_invariance_over_batches_sources_residency_and_order(gpu_ctx, tmp_path):
    import torch

    n = 2500
    pmd = _pmd("F", T=n)
    raw = _raw_movie(_exported(gpu_ctx, pmd))
    assert raw.min() >= 0 and raw.max() < 65535
    kw = dict(th=1.0, cut_off=0.5, min_size=2, ctx=gpu_ctx)
    den = localmd_amd.superpixels(pmd, **kw)
    ref = localmd_amd.superpixels(pmd, raw, kind="raw", **kw)
    assert len(den.sizes) + len(ref.sizes) > 0
    want_d, want_r = _bytes(den), _bytes(ref)
    assert want_d != want_r
    for fbs in (64, 1000):
        assert _bytes(localmd_amd.superpixels(pmd, frame_batch_size=fbs, **kw)) == want_d, fbs
        assert _bytes(localmd_amd.superpixels(pmd, raw, kind="raw", frame_batch_size=fbs, **kw)) == want_r, fbs
    u16 = raw.astype(np.uint16)
    mm = np.lib.format.open_memmap(str(tmp_path / "m.npy"), mode="w+", dtype=np.uint16, shape=raw.shape)
    mm[:] = u16
    path = str(tmp_path / "movie.tif")
    write_tiff(path, u16)
    sources = {"uint16": u16, "memmap": mm, "tiff": TiffArray(path), "cpu_tensor": torch.from_numpy(raw),
               "device_tensor": torch.from_numpy(raw).to(gpu_ctx.device)}
    for name, src in sources.items():
        assert _bytes(localmd_amd.superpixels(pmd, src, kind="raw", frame_batch_size=1024, **kw)) == want_r, name
    # threshold= reproduces the result and skips the selection rounds
    assert _bytes(localmd_amd.superpixels(pmd, threshold=den.threshold, **kw)) == want_d
    assert _bytes(localmd_amd.superpixels(pmd, u16, kind="raw", threshold=ref.threshold, **kw)) == want_r
    # device-resident factors
    pmd.to_device(ctx=gpu_ctx)
    try:
        assert _bytes(pmd.superpixels(th=1.0, cut_off=0.5, min_size=2)) == want_d
        assert _bytes(pmd.superpixels(u16, kind="raw", th=1.0, cut_off=0.5, min_size=2)) == want_r
    finally:
        pmd.to_host()
    # the same movie decomposed in C order
    pc = _pmd("C", T=n)
    assert _bytes(localmd_amd.superpixels(pc, **kw)) == want_d
    assert _bytes(localmd_amd.superpixels(pc, raw, kind="raw", **kw)) == want_r


class _Untouchable(lazy_data_loader):
    def __init__(self, shape):
        self._shape = shape

    dtype = property(lambda self: np.float32)
    shape = property(lambda self: self._shape)

    def _compute_at_indices(self, indices):
        raise AssertionError("the movie was read")


def test_reads_of_the_movie_and_bounded_memory(gpu_ctx):
    import torch

    d1 = d2 = 64
    n = 3000
    pmd = _long_pmd(n, d1, d2)
    a = localmd_amd.superpixels(pmd, min_size=2, ctx=gpu_ctx)
    b = localmd_amd.superpixels(pmd, _Untouchable((n, d1, d2)), kind="denoised", min_size=2, ctx=gpu_ctx)   # never read
    assert _bytes(a) == _bytes(b)
    src = _CountingU16(n, d1, d2)
    sp = localmd_amd.superpixels(pmd, src, kind="raw", frame_batch_size=1024, ctx=gpu_ctx)
    assert SP.movie_reads(2, "raw") == 8                                    # 3 + 4 selection passes and the moments
    assert np.all(src.count == 8), np.unique(src.count)
    src = _CountingU16(n, d1, d2)
    again = localmd_amd.superpixels(pmd, src, kind="raw", threshold=sp.threshold, frame_batch_size=1024, ctx=gpu_ctx)
    assert np.all(src.count == 1) and _bytes(again) == _bytes(sp)
    peaks = {}
    for m in (2048, 8192):
        pm = _long_pmd(m, d1, d2)
        gpu_ctx.release_workspace()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        localmd_amd.superpixels(pm, frame_batch_size=1024, ctx=gpu_ctx)
        peaks[m] = torch.cuda.max_memory_allocated() - base
    print("peak device bytes", peaks)
    assert peaks[8192] - peaks[2048] <= 1 << 20, peaks                      # the plan's slack
    tabs, xt = importlib.import_module("localmd_amd.export").expand_tables_for(pm)
    plan = SP.superpixel_device_bytes(D=d1 * d2, T=8192, nb=1024, esize=4, kind="denoised", threshold_given=False,
                                      n_cols=pm.r.shape[0], rank=pm.r.shape[1], n_entries=len(xt["entries"]),
                                      n_a=int(tabs["a"].size), n_patches=int(xt["n_patches"]), host_source=True, n_batches=8,
                                      factors_on_device=False)
    assert peaks[8192] <= plan, (peaks, plan)


# ---- planted cells -------------------------------------------------------------------------------------------------
CELLS = ((5, 5, 3.1), (6, 20, 2.9), (17, 4, 2.7), (16, 14, 3.4), (18, 17, 3.4))     # (ci, cj, radius); the last two overlap


def _planted_cells(seed=3, n=600, d1=24, d2=28):
    """A noiseless movie of five cells with Gaussian footprints on discs and traces of decaying events on a static
    background, as a PMDArray; cells 3 and 4 share 14 pixels."""
    rng = np.random.default_rng(seed)
    ii, jj = np.mgrid[0:d1, 0:d2]
    masks = np.stack([_disc(d1, d2, ci, cj, r) for ci, cj, r in CELLS])
    foot = np.stack([m * np.exp(-((ii - ci) ** 2 + (jj - cj) ** 2) / 12.0) for m, (ci, cj, r) in zip(masks, CELLS)])
    K = len(CELLS)
    traces = np.zeros((K, n))
    for k in range(K):
        for t0 in rng.choice(n - 30, 10, replace=False):
            traces[k, t0:t0 + 30] += rng.uniform(0.5, 2) * np.exp(-np.arange(30) / 6.0)
    std = rng.uniform(1, 2, (d1, d2))
    u = scipy.sparse.csr_matrix((foot.reshape(K, -1) / std.reshape(1, -1)).T)        # D x K, rows in C order
    pmd = PMDArray(u, np.eye(K, dtype=np.float32), np.ones(K, np.float32), traces.astype(np.float32), (n, d1, d2), "C",
                   rng.uniform(5, 10, (d1, d2)).astype(np.float32), std.astype(np.float32))
    return pmd, masks, traces


def test_planted_cells_are_found_and_demixed(gpu_ctx):
    """Measured on the CPU with tests/superpixel_ref.py on the host expansion of this movie (seed 3, th = 2, min_size = 4).
    cut_off = 0.9: five labels; the three isolated cells exactly (29 / 25 / 21 pixels); one label of 23 pixels inside
    cell 4 only; one of 37 pixels, all of cell 3 with the 14 shared pixels; smallest |rho - cut_off| = 2.4e-3.
    cut_off = 0.95: six labels, the shared region a 14-pixel label of its own and both cores (23 pixels each) pure;
    smallest |rho - cut_off| = 1.4e-3.  tests/hals_ref.demix_ref on those labels: the traces of the pure labels correlate
    with the planted traces at 1.000000, the mixed 37-pixel label at 0.946 with cell 3 (nothing is asserted about it)."""
    pmd, masks, traces = _planted_cells()
    assert (masks[3] & masks[4]).sum() == 14 and np.array_equal(masks.reshape(5, -1).sum(axis=1), [29, 25, 21, 37, 37])
    X = _exported(gpu_ctx, pmd)
    for cut_off, n_labels in ((0.9, 5), (0.95, 6)):
        ref = SR.superpixels_ref(X, th=2.0, cut_off=cut_off, min_size=4)
        sp = localmd_amd.superpixels(pmd, th=2.0, cut_off=cut_off, min_size=4, ctx=gpu_ctx)
        _check_against_reference(sp, ref, cut_off, ("planted", cut_off))
        assert len(sp.sizes) == n_labels
        touched = [[c for c in range(5) if (masks[c] & (sp.labels == k)).any()] for k in range(1, n_labels + 1)]
        print(cut_off, "sizes", sp.sizes, "cells touched", touched)
        assert all(t in ([0], [1], [2], [3], [4], [3, 4]) for t in touched)      # no label joins cells that do not overlap
        assert sorted(set(c for t in touched for c in t)) == [0, 1, 2, 3, 4]     # every cell is covered
        assert not (sp.labels[~masks.any(axis=0)]).any()
        for c in (0, 1, 2):
            assert np.all(sp.labels[masks[c]] > 0)
            assert len(np.unique(sp.labels[masks[c]])) == 1 and (sp.labels == sp.labels[masks[c]][0]).sum() == masks[c].sum()
        dm = pmd.demix(sp.labels, ctx=gpu_ctx)
        pure = [(k, t[0]) for k, t in enumerate(touched) if len(t) == 1]
        assert len(pure) == (4 if cut_off == 0.9 else 5)
        corr = [float(np.corrcoef(dm.traces[k], traces[c])[0, 1]) for k, c in pure]
        print(cut_off, "pure labels: correlation with the planted traces", corr)
        assert min(corr) >= 0.999
