"""ROI traces on the GPU (localmd_amd.extract_traces, csrc/roi.hip): pmd_roi_gather through the C ABI against fp64
NumPy for every element type and batch length, its independence of the batch, the end-to-end identities and bounds for
raw / denoised / residual traces, invariance over batch sizes, sources, device residency and ROI forms, a denoised-only
call that reads no movie, and a long uint16 movie traced with bounded device memory.

The fp64 references are formed here from the factors: X64 = mean + std * (U (R diag(s)) Vt), den64 = W64 X64,
raw64 = W64 Y64."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse

import localmd_amd
from localmd_amd import decomposition as Dm
from localmd_amd import traces as TR
from localmd_amd._lib import PMDLibraryError, ptr
from localmd_amd._minitiff import write_tiff
from localmd_amd.dataset import TiffArray, lazy_data_loader
from localmd_amd.pmdarray import PMDArray, load_npz, save_npz
from localmd_amd.synthetic import make_movie
from tests.consumer_fuzz import U24, factors64 as _factors64, raw_bound as _raw_bound, w64 as _w64
from tests.test_export_host import _random_tiled_u
from tests.test_traces_host import _disc, _forms, _roi_set

pytestmark = pytest.mark.gpu
Dm.QUIET = True
T, D1, D2 = 2500, 40, 44
D = D1 * D2
ALL = ("denoised", "raw", "residual")


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


def _float_weights(seed=5):
    """The ROI set of the host tests with weights that are not exactly representable in fp32."""
    w = _roi_set(D1, D2, False)
    return w * np.random.default_rng(seed).uniform(0.1, 2.0, w.shape)


# ---- the kernel through the C ABI ----------------------------------------------------------------------------------
_ELEM = {"float32": 0, "uint16": 1, "int16": 2}


def _dev(ctx, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


class _Gather:
    """Device copies of one set of ROI tables and of the movie in three containers; call() runs pmd_roi_gather on the
    frames [f0, f0 + n)."""

    def __init__(self, ctx, tabs, mov):
        self.ctx, self.t = ctx, tabs
        self.Y = {k: _dev(ctx, mov.reshape(len(mov), -1).astype(k)) for k in _ELEM}
        self.segs = _dev(ctx, tabs["segs"].reshape(-1))
        self.split = _dev(ctx, tabs["split"].reshape(-1)) if len(tabs["split"]) else None
        self.pix, self.w = _dev(ctx, tabs["pix"]), _dev(ctx, tabs["w"])

    def call(self, src, f0, n, ldo=None):
        import torch

        t, ctx = self.t, self.ctx
        ldo = n if ldo is None else ldo
        out = torch.full((t["K"], ldo), np.nan, dtype=torch.float32, device=ctx.device)
        nbytes = int(ctx.lib.pmd_roi_gather_workspace_bytes(t["n_partial_rows"], n))
        assert nbytes == 4 * t["n_partial_rows"] * n
        ws = torch.full((max(nbytes, 1),), 0xFF, dtype=torch.uint8, device=ctx.device)
        y = self.Y[src]
        yp = C.c_void_p(y.data_ptr() + f0 * t["D"] * y.element_size())
        ctx.call("pmd_roi_gather", yp, _ELEM[src], n, t["D"], len(t["segs"]), ptr(self.segs), ptr(self.pix), ptr(self.w),
                 t["n_partial_rows"], len(t["split"]), ptr(self.split), ptr(out), ldo, ptr(ws), nbytes)
        ctx.sync()
        return out.cpu().numpy()


@pytest.mark.parametrize("seg", [TR.ROI_SEG, 128])
@pytest.mark.parametrize("order", ["F", "C"])
def test_gather_boolean_masks_exact_for_every_container_and_length(gpu_ctx, case, order, seg):
    mov = case[0]
    Y64 = mov.reshape(T, D).astype(np.float64)
    assert mov.min() >= 0 and mov.max() <= 32767 and np.array_equal(mov, np.rint(mov))   # exact in all three containers
    w = _roi_set(D1, D2, False)
    tabs = TR.roi_tables(_forms(w, order)["sparse"], (D1, D2), order, "sum", seg=seg)
    W64 = _w64(w, "sum")
    assert (W64 != 0).sum(axis=1).max() == D and D * np.abs(Y64).max() < 2 ** 24         # every partial sum is exact
    assert len(tabs["split"]) >= 1
    g = _Gather(gpu_ctx, tabs, mov)
    f0 = 1100
    for n in (1, 63, 64, 65, 1000):
        want = W64 @ Y64[f0:f0 + n].T
        got = {src: g.call(src, f0, n) for src in _ELEM}
        print("n", n, "max |got - raw64|", np.abs(got["float32"] - want).max())
        assert np.array_equal(got["float32"].astype(np.float64), want), n
        assert got["uint16"].tobytes() == got["float32"].tobytes() and got["int16"].tobytes() == got["float32"].tobytes()
    padded = g.call("uint16", f0, 65, ldo=72)                                            # a leading dimension > n
    assert np.array_equal(padded[:, :65].astype(np.float64), W64 @ Y64[f0:f0 + 65].T) and np.all(np.isnan(padded[:, 65:]))


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_gather_float_weights_within_the_forward_bound(gpu_ctx, case, reduce):
    mov = case[0]
    Y64 = mov.reshape(T, D).astype(np.float64)
    w = _float_weights()
    tabs = TR.roi_tables(w, (D1, D2), "F", reduce)
    W64 = _w64(w, reduce)
    g = _Gather(gpu_ctx, tabs, mov)
    for n in (1, 63, 64, 65, 1000):
        want = W64 @ Y64[:n].T
        bound = _raw_bound(W64, Y64[:n].T)
        got = {src: g.call(src, 0, n) for src in _ELEM}
        ratio = np.abs(got["float32"] - want) / bound
        print("n", n, "max error / bound", ratio.max())
        assert np.all(np.abs(got["float32"] - want) <= bound), (n, ratio.max())
        assert got["uint16"].tobytes() == got["float32"].tobytes() and got["int16"].tobytes() == got["float32"].tobytes()


@pytest.mark.parametrize("split", [1, 37, 64, 700])
def test_gather_split_calls_are_bitwise_equal(gpu_ctx, case, split):
    mov = case[0]
    tabs = TR.roi_tables(_float_weights(), (D1, D2), "C", "mean")
    g = _Gather(gpu_ctx, tabs, mov)
    n = 1030
    for src in ("float32", "uint16"):
        whole = g.call(src, 200, n)
        parts = np.concatenate([g.call(src, 200, split), g.call(src, 200 + split, n - split)], axis=1)
        assert whole.tobytes() == parts.tobytes()


def test_kernel_rejects_bad_arguments(gpu_ctx):
    with pytest.raises((PMDLibraryError, RuntimeError)):
        gpu_ctx.call("pmd_roi_gather", None, 7, 4, 35, 1, None, None, None, 0, 0, None, None, 4, None, 0)   # element type
    with pytest.raises((PMDLibraryError, RuntimeError)):
        gpu_ctx.call("pmd_roi_gather", None, 0, 4, 35, 1, None, None, None, 0, 0, None, None, 3, None, 0)   # ldo < n
    with pytest.raises((PMDLibraryError, RuntimeError)):
        gpu_ctx.call("pmd_roi_gather", None, 0, 4, 35, 1, None, None, None, 2, 0, None, None, 4, None, 0)   # rows, no split
    with pytest.raises((PMDLibraryError, RuntimeError)):
        gpu_ctx.call("pmd_roi_combine", -1, 4, None, 4, None, None, 4, None, 4, None, 4)                     # K < 0


# ---- end to end ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("order", ["F", "C"])
def test_traces_against_fp64(gpu_ctx, case, order, reduce):
    mov, pmds = case
    pmd = pmds[order]
    Y64 = mov.reshape(T, D).astype(np.float64).T                              # (D, T)
    mean, std, uc, rs, vt = _factors64(pmd)
    X64 = mean[:, None] + std[:, None] * (uc @ rs @ vt)
    absX = np.abs(mean)[:, None] + std[:, None] * (np.abs(uc) @ np.abs(rs) @ np.abs(vt))
    # boolean masks: raw is exact under "sum"
    wb = _roi_set(D1, D2, False)
    if reduce == "sum":
        tr = localmd_amd.extract_traces(pmd, wb.astype(bool), mov, kinds=ALL, reduce="sum", frame_batch_size=1024,
                                        ctx=gpu_ctx)
        W64 = _w64(wb, "sum")
        assert D * np.abs(Y64).max() < 2 ** 24
        assert np.array_equal(tr.raw.astype(np.float64), W64 @ Y64)
        assert np.array_equal(tr.residual, tr.raw - tr.denoised)
        assert np.all(np.abs(tr.denoised - W64 @ X64) <= 1e-5 * (np.abs(W64) @ absX) + 1e-6)
    # float weights: the forward bounds
    w = _float_weights()
    W64 = _w64(w, reduce)
    tr = pmd.traces(w, mov, kinds=ALL, reduce=reduce, frame_batch_size=1024, ctx=gpu_ctx)
    assert np.array_equal(tr.labels, np.arange(w.shape[0]))
    for a in (tr.denoised, tr.raw, tr.residual):
        assert a.shape == (w.shape[0], T) and a.dtype == np.float32
    raw64, den64 = W64 @ Y64, W64 @ X64
    rb = _raw_bound(W64, Y64)
    db = 1e-5 * (np.abs(W64) @ absX) + 1e-6
    print("raw: max error / bound", (np.abs(tr.raw - raw64) / rb).max(), "denoised:", (np.abs(tr.denoised - den64) / db).max())
    assert np.all(np.abs(tr.raw - raw64) <= rb)
    assert np.all(np.abs(tr.denoised - den64) <= db)
    assert np.array_equal(tr.residual, tr.raw - tr.denoised)


@pytest.mark.parametrize("order", ["F", "C"])
def test_one_pixel_roi_agrees_with_getitem(gpu_ctx, case, order):
    mov, pmds = case
    pmd = pmds[order]
    mean, std, uc, rs, vt = _factors64(pmd)
    scale = np.abs(mean[:, None] + std[:, None] * (uc @ rs @ vt)).max()
    pts = [(0, 0), (17, 23), (D1 - 1, D2 - 1), (5, 40)]
    rois = np.zeros((len(pts), D1, D2), bool)
    for k, (i, j) in enumerate(pts):
        rois[k, i, j] = True
    for reduce in ("mean", "sum"):
        tr = localmd_amd.extract_traces(pmd, rois, kinds="denoised", reduce=reduce, ctx=gpu_ctx)
        assert tr.raw is None and tr.residual is None
        for k, (i, j) in enumerate(pts):
            ref = np.asarray(pmd[:, i, j], np.float32).reshape(-1)
            assert np.max(np.abs(tr.denoised[k] - ref)) < 4e-6 * scale, (i, j)
    raw = localmd_amd.extract_traces(pmd, rois, mov, kinds="raw", reduce="mean", ctx=gpu_ctx).raw
    for k, (i, j) in enumerate(pts):
        assert np.array_equal(raw[k], mov[:, i, j])


def _bytes(tr):
    return tr.denoised.tobytes() + tr.raw.tobytes() + tr.residual.tobytes()


def test_batch_source_residency_and_form_invariance(gpu_ctx, case, tmp_path):
    import torch

    mov, pmds = case
    pmd = pmds["F"]
    w = _float_weights()
    want = _bytes(localmd_amd.extract_traces(pmd, w, mov, kinds=ALL, frame_batch_size=1024, ctx=gpu_ctx))
    for fbs in (100, 1024, 10000):
        got = localmd_amd.extract_traces(pmd, w, mov, kinds=ALL, frame_batch_size=fbs, ctx=gpu_ctx)
        assert _bytes(got) == want, fbs
    u16 = mov.astype(np.uint16)
    mm = np.lib.format.open_memmap(str(tmp_path / "m.npy"), mode="w+", dtype=np.uint16, shape=mov.shape)
    mm[:] = u16
    path = str(tmp_path / "movie.tif")
    write_tiff(path, u16)
    sources = {"numpy_u16": u16, "memmap": mm, "cpu_tensor": torch.from_numpy(mov), "tiff": TiffArray(path),
               "device_tensor": torch.from_numpy(mov).to(gpu_ctx.device),
               "device_i16": torch.from_numpy(mov.astype(np.int16)).to(gpu_ctx.device)}
    for name, src in sources.items():
        got = localmd_amd.extract_traces(pmd, w, src, kinds=ALL, frame_batch_size=2048, ctx=gpu_ctx)
        assert _bytes(got) == want, name
    # kinds in another order, and one at a time
    got = localmd_amd.extract_traces(pmd, w, mov, kinds=("residual", "raw", "denoised"), ctx=gpu_ctx)
    assert _bytes(got) == want
    only_res = localmd_amd.extract_traces(pmd, w, u16, kinds="residual", frame_batch_size=1024, ctx=gpu_ctx)
    assert only_res.raw is None and only_res.denoised is None and only_res.residual.tobytes() == got.residual.tobytes()
    # device-resident factors
    pmd.to_device(ctx=gpu_ctx)
    try:
        got = pmd.traces(w, mov, kinds=ALL)
    finally:
        pmd.to_host()
    assert _bytes(got) == want
    # a decomposition read back from disk
    npz = str(tmp_path / "pmd.npz")
    save_npz(npz, pmd)
    got = localmd_amd.extract_traces(load_npz(npz), w, mov, kinds=ALL, ctx=gpu_ctx)
    assert _bytes(got) == want
    # the three ROI forms
    for order in ("F", "C"):
        p = pmds[order]
        ref = _bytes(localmd_amd.extract_traces(p, w, mov, kinds=ALL, ctx=gpu_ctx))
        for name, rois in _forms(w, order).items():
            assert _bytes(localmd_amd.extract_traces(p, rois, mov, kinds=ALL, ctx=gpu_ctx)) == ref, (order, name)
        lab = np.zeros((D1, D2), np.int64)
        lab[_disc(D1, D2, 20, 20, 5)] = 9
        lab[_disc(D1, D2, 8, 30, 4)] = 2
        lab[35:, :] = 4
        a = localmd_amd.extract_traces(p, lab, mov, kinds=ALL, ctx=gpu_ctx)
        b = localmd_amd.extract_traces(p, np.stack([lab == v for v in (2, 4, 9)]), mov, kinds=ALL, ctx=gpu_ctx)
        assert np.array_equal(a.labels, [2, 4, 9]) and np.array_equal(b.labels, [0, 1, 2])
        assert _bytes(a) == _bytes(b)


class _Untouchable(lazy_data_loader):
    dtype = property(lambda self: np.float32)
    shape = property(lambda self: (T, D1, D2))

    def _compute_at_indices(self, indices):
        raise AssertionError("the movie was read")


def test_denoised_only_reads_no_movie(gpu_ctx, case):
    mov, pmds = case
    pmd = pmds["C"]
    w = _float_weights()
    a = localmd_amd.extract_traces(pmd, w, ctx=gpu_ctx)                              # kinds defaults to ("denoised",)
    b = localmd_amd.extract_traces(pmd, w, _Untouchable(), kinds=("denoised",), ctx=gpu_ctx)
    c = localmd_amd.extract_traces(pmd, w, mov, kinds=ALL, ctx=gpu_ctx)
    assert a.raw is None and a.residual is None and b.raw is None
    assert a.denoised.tobytes() == b.denoised.tobytes() == c.denoised.tobytes()


def test_background_rank_zero_and_no_components(gpu_ctx, case):
    mov = case[0]
    pmd = _decompose(gpu_ctx, mov, "F", background_rank=0)
    w = _float_weights()
    W64 = _w64(w, "mean")
    mean, std, uc, rs, vt = _factors64(pmd)
    den64 = W64 @ (mean[:, None] + std[:, None] * (uc @ rs @ vt))
    tr = localmd_amd.extract_traces(pmd, w, ctx=gpu_ctx)
    assert np.max(np.abs(tr.denoised - den64)) < 2e-6 * np.abs(den64).max()
    # rank 0: the denoised movie is the mean image
    empty = PMDArray(scipy.sparse.csr_matrix((D, 0)), np.zeros((0, 0), np.float32), np.zeros(0, np.float32),
                     np.zeros((0, T), np.float32), (T, D1, D2), "F", pmd.mean_img, pmd.var_img)
    tr = localmd_amd.extract_traces(empty, w, mov, kinds=ALL, ctx=gpu_ctx)
    off = (W64 @ mean).astype(np.float32)
    assert np.array_equal(tr.denoised, np.repeat(off[:, None], T, axis=1))
    assert np.array_equal(tr.residual, tr.raw - tr.denoised)


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

    d1, d2 = 128, 128
    rng = np.random.default_rng(8)
    masks = [_disc(d1, d2, int(rng.integers(6, d1 - 6)), int(rng.integers(6, d2 - 6)), 4.6) for _ in range(199)]
    rois = np.stack(masks + [np.ones((d1, d2), bool)])                     # 199 discs and the whole field
    W64 = _w64(rois, "mean")
    peaks = {}
    for n in (10000, 40000):
        src = _CountingU16(n, d1, d2)
        pmd = _long_pmd(n, d1, d2)
        gpu_ctx.release_workspace()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        tr = localmd_amd.extract_traces(pmd, rois, src, kinds=ALL, frame_batch_size=4096, ctx=gpu_ctx)
        peaks[n] = torch.cuda.max_memory_allocated() - base
        assert np.all(src.count == 1), np.unique(src.count)
        t = TR.roi_tables(rois, (d1, d2), "F", "mean")
        B, _ = TR.denoised_factors(pmd, t["W"])
        est = TR.traces_device_bytes(d1 * d2, 4096, 2, len(rois), 3, 0, t["pix"].size, len(t["segs"]), len(t["split"]),
                                     t["n_partial_rows"], B.nnz, pmd.u.shape[1], 12, True, True, -(-n // 4096), False)
        assert peaks[n] <= est, (peaks[n], est)
        keep = np.array([0, 1023, 1024, 4095, 4096, n // 2 + 7, n - 1])
        y64 = src.frames(keep).reshape(len(keep), -1).astype(np.float64).T
        raw64 = W64 @ y64
        assert np.all(np.abs(tr.raw[:, keep] - raw64) <= _raw_bound(W64, y64))
        x = np.asarray(pmd[list(keep)], np.float64).reshape(len(keep), -1).T
        np.testing.assert_allclose(tr.denoised[:, keep], W64 @ x, rtol=1e-5, atol=1e-3)
        assert np.array_equal(tr.residual, tr.raw - tr.denoised)
    assert peaks[40000] - peaks[10000] <= 1 << 20, peaks
