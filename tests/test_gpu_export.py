"""Streamed export on the GPU (localmd_amd.export_movie, csrc/expand_fused.hip): pmd_group_expand through the C ABI
against fp64 NumPy for every element type and panel set, its determinism and conversion, the end-to-end identities,
invariance over batch sizes, sources and destinations, and a long uint16 movie exported with bounded device memory."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse

import localmd_amd
from localmd_amd import decomposition as Dm
from localmd_amd import export as E
from localmd_amd import projection as P
from localmd_amd._lib import ptr
from localmd_amd._minitiff import write_tiff
from localmd_amd.dataset import TiffArray, lazy_data_loader
from localmd_amd.pmdarray import PMDArray, load_npz, save_npz
from localmd_amd.synthetic import make_movie
from tests.consumer_fuzz import recon64 as _recon64
from tests.test_export_host import _random_tiled_u
from tests.util import degenerate_pmds

pytestmark = pytest.mark.gpu
Dm.QUIET = True
T, D1, D2 = 2500, 40, 44
TRIPTYCH = ("raw", "denoised", "residual")


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


# ---- the kernel through the C ABI ----------------------------------------------------------------------------------
_ELEM = {"float32": 0, "uint16": 1, "int16": 2}


def _dev(ctx, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


class _Kernel:
    """Device copies of one set of tables, C, Y, mean and std; call() runs pmd_group_expand on frames [f0, f0 + n)."""

    def __init__(self, ctx, u, fov, order, Cm, Y, mean, std):
        self.ctx = ctx
        self.d1, self.d2 = fov
        self.tabs = P.group_tables(u, fov, order)
        self.xt = E.expand_tables(self.tabs)
        E.validate_expand_tables(self.xt, self.tabs["a"].size, self.tabs["n_cols"], self.tabs["D"])
        self.n_ent = len(self.xt["entries"])
        self.ldc = Cm.shape[1]
        self.C = _dev(ctx, Cm.astype(np.float32)) if Cm.shape[0] else None
        self.Y = {k: _dev(ctx, v) for k, v in Y.items()}
        self.mean, self.std = _dev(ctx, mean.astype(np.float32)), _dev(ctx, std.astype(np.float32))
        self.pp = _dev(ctx, self.xt["patch_ptr"])
        self.ent = _dev(ctx, self.xt["entries"].reshape(-1)) if self.n_ent else None
        self.qm = _dev(ctx, self.xt["qmap"]) if self.n_ent else None
        self.A = _dev(ctx, self.tabs["a"]) if self.n_ent else None

    def call(self, src, out_dtype, panels, f0, n, out=None):
        import torch

        D = self.d1 * self.d2
        Pn = len(panels)
        code = sum(E._PANEL_CODE[p] << (2 * k) for k, p in enumerate(panels))
        isz = np.dtype(out_dtype).itemsize
        fb = D * Pn * isz
        if out is None:
            out = torch.full((n * fb,), 0x7F, dtype=torch.uint8, device=self.ctx.device)
        y = self.Y[src]
        cp = C.c_void_p(self.C.data_ptr() + 4 * f0) if self.C is not None else None
        yp = C.c_void_p(y.data_ptr() + f0 * D * y.element_size())
        self.ctx.call("pmd_group_expand", cp, self.ldc, n, self.d1, self.d2, ptr(self.mean), ptr(self.std),
                      int(self.xt["n_patches"]), ptr(self.pp), self.n_ent, ptr(self.ent), ptr(self.qm), ptr(self.A), yp,
                      _ELEM[src], D, Pn, code, C.c_void_p(out.data_ptr()), _ELEM[out_dtype])
        return out

    def host(self, out, out_dtype, panels, n):
        self.ctx.sync()
        return out.cpu().numpy().view(np.dtype(out_dtype)).reshape(n, self.d1, len(panels) * self.d2)


@pytest.mark.parametrize("which", ["no_columns", "rank_zero"])
def test_decomposition_without_columns_or_rank_exports_the_mean_image(gpu_ctx, case, which):
    """Nothing to expand (no entries) and nothing to multiply (rank 0, C stays zero): x = mean, r = y - mean."""
    mov, pmds = case
    pmd = degenerate_pmds(pmds["C"])[which]
    mean = np.asarray(pmd.mean_img, np.float32)
    want = np.concatenate([mov, np.broadcast_to(mean, mov.shape), mov - mean[None]], axis=2)
    for src in (mov, mov.astype(np.uint16)):
        got = np.empty_like(want)
        localmd_amd.export_movie(pmd, got, src, panels=TRIPTYCH, frame_batch_size=1024, ctx=gpu_ctx)
        assert got.tobytes() == want.tobytes()
    den = np.empty((T, D1, D2), np.uint16)
    localmd_amd.export_movie(pmd, den, panels="denoised", dtype="uint16", ctx=gpu_ctx)
    assert np.array_equal(den, np.broadcast_to(E.quantize(mean, np.uint16), den.shape))


def _tables_case(kind, gpu_ctx, case):
    """(u, fov, order) of the four table sources."""
    if kind == "decomposition":
        pmd = case[1]["C"]
        return pmd.u, (D1, D2), "C"
    if kind == "merged_empty_rows":
        return _random_tiled_u(31, 37, 10, 8, "F", 2, seed=9, merged=True, empty_rows=True), (31, 37), "F"
    if kind == "only_wide":
        rng = np.random.default_rng(2)
        return scipy.sparse.csr_matrix(rng.standard_normal((45 * 50, 3))), (45, 50), "C"
    return scipy.sparse.csr_matrix((23 * 37, 0)), (23, 37), "F"


def _sources(n, D, seed):
    rng = np.random.default_rng(seed)
    return {"float32": (rng.standard_normal((n, D)) * 50 + 900).astype(np.float32),
            "uint16": rng.integers(0, 4000, (n, D)).astype(np.uint16),
            "int16": rng.integers(-2000, 2000, (n, D)).astype(np.int16)}


@pytest.mark.parametrize("n", [1, 5, 1023, 1030])
@pytest.mark.parametrize("kind", ["decomposition", "merged_empty_rows", "only_wide", "no_columns"])
def test_kernel_against_fp64(gpu_ctx, case, kind, n):
    u, fov, order = _tables_case(kind, gpu_ctx, case)
    D = fov[0] * fov[1]
    rng = np.random.default_rng(n)
    Cm = (rng.standard_normal((u.shape[1], n)) * 3).astype(np.float32)
    mean = (rng.standard_normal(D) * 100 + 900).astype(np.float32)
    std = rng.uniform(0.5, 20, D).astype(np.float32)
    Y = _sources(n, D, n + 1)
    k = _Kernel(gpu_ctx, u, fov, order, Cm, Y, mean, std)
    u_of_c = np.arange(D).reshape(fov, order=order).reshape(-1)
    uc = u.astype(np.float32).astype(np.float64)[u_of_c]
    acc = (uc @ Cm.astype(np.float64)).T                                    # (n, D)
    x64 = mean.astype(np.float64) + std.astype(np.float64) * acc
    bound = 1e-5 * (np.abs(mean) + std * (np.abs(uc) @ np.abs(Cm.astype(np.float64))).T) + 1e-6
    for src, y in Y.items():
        y32 = y.astype(np.float32)
        for panels in [("denoised",), TRIPTYCH, ("residual", "raw")]:
            got32 = k.host(k.call(src, "float32", panels, 0, n), "float32", panels, n)
            pan = {p: got32[:, :, j * fov[1]:(j + 1) * fov[1]].reshape(n, D) for j, p in enumerate(panels)}
            if "raw" in pan:
                assert np.array_equal(pan["raw"], y32)
            if "denoised" in pan:
                assert np.all(np.abs(pan["denoised"] - x64) <= bound), (kind, src, np.max(np.abs(pan["denoised"] - x64)))
                if "residual" in pan:
                    assert np.array_equal(pan["residual"], y32 - pan["denoised"])
            if "residual" in pan:
                assert np.all(np.abs(pan["residual"] - (y32 - x64)) <= bound + 1e-4 * np.abs(y32))
            for odt in ("uint16", "int16"):
                goti = k.host(k.call(src, odt, panels, 0, n), odt, panels, n)
                assert np.array_equal(goti, E.quantize(got32, odt)), (kind, src, odt, panels)


@pytest.mark.parametrize("split", [1, 37, 64, 700])
def test_kernel_split_calls_are_bitwise_equal(gpu_ctx, case, split):
    import torch

    u, fov, order = _tables_case("merged_empty_rows", gpu_ctx, case)
    D = fov[0] * fov[1]
    n = 1030
    rng = np.random.default_rng(3)
    Cm = rng.standard_normal((u.shape[1], n)).astype(np.float32)
    k = _Kernel(gpu_ctx, u, fov, order, Cm, _sources(n, D, 4), rng.standard_normal(D) * 50, rng.uniform(1, 5, D))
    for src in ("float32", "uint16"):
        whole = k.host(k.call(src, "float32", TRIPTYCH, 0, n), "float32", TRIPTYCH, n)
        fb = D * 3 * 4
        out = torch.full((n * fb,), 0x7F, dtype=torch.uint8, device=gpu_ctx.device)
        k.call(src, "float32", TRIPTYCH, 0, split, out=out[:split * fb])
        k.call(src, "float32", TRIPTYCH, split, n - split, out=out[split * fb:])
        parts = k.host(out, "float32", TRIPTYCH, n)
        assert whole.tobytes() == parts.tobytes()


def test_kernel_rejects_bad_arguments(gpu_ctx):
    from localmd_amd._lib import PMDLibraryError

    with pytest.raises((PMDLibraryError, RuntimeError)):
        gpu_ctx.call("pmd_group_expand", None, 4, 4, 5, 7, None, None, 2, None, 0, None, None, None, None, 0, 35, 4, 0,
                     None, 0)       # four panels


# ---- end to end ----------------------------------------------------------------------------------------------------
def _panel(a, k, d2=D2):
    return a[:, :, k * d2:(k + 1) * d2]


@pytest.mark.parametrize("order", ["F", "C"])
def test_triptych_identities(gpu_ctx, case, order):
    mov, pmds = case
    pmd = pmds[order]
    out = np.empty((T, D1, 3 * D2), np.float32)
    got = localmd_amd.export_movie(pmd, out, mov, panels=TRIPTYCH, frame_batch_size=1024, ctx=gpu_ctx)
    assert got is out
    raw, den, res = _panel(out, 0), _panel(out, 1), _panel(out, 2)
    assert np.array_equal(raw, mov)
    assert np.array_equal(res, raw - den)
    x64 = _recon64(pmd)
    scale = np.abs(x64).max()
    assert np.max(np.abs(den - x64)) < 2e-6 * scale, np.max(np.abs(den - x64)) / scale
    ref = np.asarray(pmd[0:T], np.float32)
    assert np.max(np.abs(den - ref)) < 4e-6 * scale


def test_batch_and_source_invariance(gpu_ctx, case, tmp_path):
    import torch

    mov, pmds = case
    pmd = pmds["F"]
    want = np.empty((T, D1, 3 * D2), np.float32)
    localmd_amd.export_movie(pmd, want, mov, panels=TRIPTYCH, frame_batch_size=1024, ctx=gpu_ctx)
    for fbs in (3072, 10 ** 6):
        got = np.empty_like(want)
        localmd_amd.export_movie(pmd, got, mov, panels=TRIPTYCH, frame_batch_size=fbs, ctx=gpu_ctx)
        assert got.tobytes() == want.tobytes(), fbs
    u16 = np.lib.format.open_memmap(str(tmp_path / "m.npy"), mode="w+", dtype=np.uint16, shape=mov.shape)
    u16[:] = mov.astype(np.uint16)
    path = str(tmp_path / "movie.tif")
    write_tiff(path, mov.astype(np.uint16))
    sources = {"u16_memmap": u16, "tiff": TiffArray(path), "cpu_tensor": torch.from_numpy(mov),
               "device_tensor": torch.from_numpy(mov).to(gpu_ctx.device),
               "device_i16": torch.from_numpy(mov.astype(np.int16)).to(gpu_ctx.device)}
    for name, src in sources.items():
        got = np.empty_like(want)
        localmd_amd.export_movie(pmd, got, src, panels=TRIPTYCH, frame_batch_size=3072, ctx=gpu_ctx)
        assert got.tobytes() == want.tobytes(), name


def test_destinations_hold_the_same_bits(gpu_ctx, case, tmp_path):
    import torch

    mov, pmds = case
    pmd = pmds["C"]
    panels = ("denoised", "residual")
    for dtype in ("float32", "uint16"):
        want = np.empty((T, D1, 2 * D2), np.dtype(dtype))
        localmd_amd.export_movie(pmd, want, mov, panels=panels, dtype=dtype, ctx=gpu_ctx)
        if dtype == "uint16":
            f = np.empty((T, D1, 2 * D2), np.float32)
            localmd_amd.export_movie(pmd, f, mov, panels=panels, ctx=gpu_ctx)
            assert np.array_equal(want, E.quantize(f, "uint16"))
        for big in (None, True):
            p = str(tmp_path / "o_{}_{}.tif".format(dtype, big))
            assert localmd_amd.export_movie(pmd, p, mov, panels=panels, dtype=dtype, bigtiff=big, ctx=gpu_ctx) == p
            with open(p, "rb") as fh:
                assert fh.read(4)[2] == (43 if big else 42)
            back = TiffArray(p)
            assert back.shape == want.shape
            assert np.array_equal(np.asarray(back[0:T]), want.astype(np.float32))
        p = str(tmp_path / "o_{}.npy".format(dtype))
        pmd.export(p, mov, panels=panels, dtype=dtype, ctx=gpu_ctx)
        assert np.load(p).tobytes() == want.tobytes()
        td = getattr(torch, dtype)
        dt = torch.empty((T, D1, 2 * D2), dtype=td, device=gpu_ctx.device)
        p0 = dt.data_ptr()
        assert localmd_amd.export_movie(pmd, dt, mov, panels=panels, dtype=dtype, ctx=gpu_ctx) is dt
        assert dt.data_ptr() == p0
        assert dt.cpu().numpy().tobytes() == want.tobytes()
        ct = torch.empty((T, D1, 2 * D2), dtype=td)
        localmd_amd.export_movie(pmd, ct, mov, panels=panels, dtype=dtype, ctx=gpu_ctx)
        assert ct.numpy().tobytes() == want.tobytes()


def test_failed_export_removes_its_file(gpu_ctx, case, tmp_path):
    """A movie whose reader fails midway: the error reaches the caller and the half-written TIFF is gone."""
    mov, pmds = case

    class Failing(lazy_data_loader):
        dtype = property(lambda self: np.float32)
        shape = property(lambda self: mov.shape)

        def _compute_at_indices(self, indices):
            idx = np.arange(T)[indices].reshape(-1)
            if idx.max() >= 2048:
                raise OSError("read error")
            return mov[idx]

    p = tmp_path / "f.tif"
    with pytest.raises(OSError):
        localmd_amd.export_movie(pmds["F"], str(p), Failing(), panels=TRIPTYCH, frame_batch_size=1024, ctx=gpu_ctx)
    assert not p.exists()


def test_device_resident_and_loaded_pmdarray(gpu_ctx, case, tmp_path):
    mov, pmds = case
    pmd = pmds["F"]
    want = np.empty((T, D1, 3 * D2), np.float32)
    localmd_amd.export_movie(pmd, want, mov, panels=TRIPTYCH, ctx=gpu_ctx)
    pmd.to_device(ctx=gpu_ctx)
    try:
        got = np.empty_like(want)
        pmd.export(got, mov, panels=TRIPTYCH)
    finally:
        pmd.to_host()
    assert got.tobytes() == want.tobytes()
    path = str(tmp_path / "pmd.npz")
    save_npz(path, pmd)
    loaded = load_npz(path)
    got = np.empty_like(want)
    localmd_amd.export_movie(loaded, got, mov, panels=TRIPTYCH, ctx=gpu_ctx)
    assert got.tobytes() == want.tobytes()


def test_background_rank_zero(gpu_ctx, case):
    mov = case[0]
    pmd = _decompose(gpu_ctx, mov, "F", background_rank=0)
    out = np.empty((T, D1, D2), np.float32)
    localmd_amd.export_movie(pmd, out, ctx=gpu_ctx)
    x64 = _recon64(pmd)
    assert np.max(np.abs(out - x64)) < 2e-6 * np.abs(x64).max()


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


class _Discard:
    """Destination that keeps nothing: checks that frames arrive once and in order, keeps a few."""

    def __init__(self, shape, keep):
        self.shape, self.dtype = shape, np.dtype(np.float32)
        self.next, self.keep, self.kept = 0, set(keep), {}

    def __setitem__(self, key, block):
        assert key.start == self.next and key.stop - key.start == len(block)
        for t in self.keep & set(range(key.start, key.stop)):
            self.kept[t] = np.array(block[t - key.start])
        self.next = key.stop


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
    peaks = {}
    for n in (10000, 40000):
        src = _CountingU16(n, d1, d2)
        pmd = _long_pmd(n, d1, d2)
        keep = [0, 1023, 1024, n // 2 + 7, n - 1]
        sink = _Discard((n, d1, 3 * d2), keep)
        gpu_ctx.release_workspace()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        assert localmd_amd.export_movie(pmd, sink, src, panels=TRIPTYCH, frame_batch_size=4096, ctx=gpu_ctx) is sink
        peaks[n] = torch.cuda.max_memory_allocated() - base
        assert np.all(src.count == 1), np.unique(src.count)
        assert sink.next == n
        tabs, xt = E.expand_tables_for(pmd)
        est = E.export_device_bytes(d1 * d2, 4096, 2, 3, 4, pmd.u.shape[1], 12, len(xt["entries"]), tabs["a"].size,
                                    xt["n_patches"], True, True, -(-n // 4096), True, False)
        assert peaks[n] <= est, (peaks[n], est)
        idx = np.array(keep)
        y = src.frames(idx).astype(np.float32)
        x = np.asarray(pmd[keep], np.float32)
        for j, t in enumerate(keep):
            f = sink.kept[t]
            assert np.array_equal(f[:, :d2], y[j])
            np.testing.assert_allclose(f[:, d2:2 * d2], x[j], rtol=1e-5, atol=1e-3)
            assert np.array_equal(f[:, 2 * d2:], f[:, :d2] - f[:, d2:2 * d2])
    assert peaks[40000] - peaks[10000] <= 1 << 20, peaks
