"""One-pass fit diagnostics on the GPU (localmd_amd.make_pmd_diagnostic_images, csrc/diag_fused.hip): all seven fields
against fp64 NumPy and against the four existing image routines, invariance over batch sizes and sources, and a long
uint16 movie read once with bounded device memory."""
import os
import warnings

import numpy as np
import pytest

import localmd_amd
from localmd_amd import decomposition as Dm
from localmd_amd import diagnostic_images as DI
from localmd_amd.dataset import TiffArray, lazy_data_loader
from localmd_amd._minitiff import write_tiff
from localmd_amd.synthetic import make_movie
from oracle import diag_oracle as DO

pytestmark = pytest.mark.gpu
Dm.QUIET = True
T, D1, D2 = 2500, 40, 44


def _int_movie(seed):
    """Integer-valued fp32 movie (exact in uint16): mean about 900, noise std about 8."""
    return np.rint(8.0 * make_movie(T, D1, D2, seed=seed)).astype(np.float32)


def _decompose(ctx, mov, order):
    np.random.seed(0)
    return localmd_amd.localmd_decomposition(mov, (20, 20), 1000, max_components=4, background_rank=1, seed=3, sim_iters=5,
                                             order=order, ctx=ctx)


@pytest.fixture(scope="module")
def case(gpu_ctx):
    mov = _int_movie(4)
    return mov, {o: _decompose(gpu_ctx, mov, o) for o in ("F", "C")}


def _fp64_fields(mov, pmd, mode, lag):
    y = mov.astype(np.float64)
    x = np.asarray(pmd[:, :, :], dtype=np.float64)
    r = y - x
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        var_y = y.var(axis=0)
        ev = np.where(var_y > 0, 1.0 - r.var(axis=0) / np.where(var_y > 0, var_y, 1.0), np.nan)
        return (DO.make_correlation_image(y, mode), DO.make_autocorrelation_image(y, lag),
                DO.make_pmd_correlation_image(y, x, mode), DO.make_residual_correlation_image(y, x, mode),
                r.std(axis=0), ev, np.sqrt((r ** 2).mean(axis=(1, 2))))


def _check_close(got, want):
    names = DI.PMDDiagnostics._fields
    tol = {"correlation": (1e-5, 1e-6), "autocorrelation": (1e-5, 1e-6), "pmd_correlation": (1e-4, 1e-5),
           "residual_correlation": (1e-3, 1e-5), "residual_std": (1e-4, 1e-5), "explained_variance": (1e-4, 1e-5),
           "frame_residual_rms": (1e-4, 1e-6)}
    for name, g, w in zip(names, got, want):
        assert g.dtype == np.float64 and g.shape == np.shape(w), name
        rtol, atol = tol[name]
        np.testing.assert_allclose(g, w, rtol=rtol, atol=atol, err_msg=name)


def _assert_same(a, b):
    for name, x, y in zip(DI.PMDDiagnostics._fields, a, b):
        np.testing.assert_array_equal(x, y, err_msg=name)


@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("lag", [1, 3])
@pytest.mark.parametrize("mode", ["max", "mean"])
def test_against_fp64(gpu_ctx, case, order, lag, mode):
    mov, pmds = case
    pmd = pmds[order]
    got = localmd_amd.make_pmd_diagnostic_images(mov, pmd, mode=mode, lag=lag, frame_batch_size=1024, ctx=gpu_ctx)
    assert isinstance(got, DI.PMDDiagnostics) and got.frame_residual_rms.shape == (T,)
    _check_close(got, _fp64_fields(mov, pmd, mode, lag))


def test_projected_movie_against_fp64(gpu_ctx, case):
    mov, pmds = case
    mov2 = _int_movie(9)
    pmd2 = localmd_amd.project_movie(pmds["F"], mov2, ctx=gpu_ctx)
    got = localmd_amd.make_pmd_diagnostic_images(mov2, pmd2, mode="mean", lag=2, frame_batch_size=2048, ctx=gpu_ctx)
    _check_close(got, _fp64_fields(mov2, pmd2, "mean", 2))


def test_device_resident_pmdarray(gpu_ctx, case):
    mov, pmds = case
    pmd = pmds["C"]
    want = localmd_amd.make_pmd_diagnostic_images(mov, pmd, lag=3, frame_batch_size=1024, ctx=gpu_ctx)
    pmd.to_device(ctx=gpu_ctx)
    try:
        got = localmd_amd.make_pmd_diagnostic_images(mov, pmd, lag=3, frame_batch_size=1024)
    finally:
        pmd.to_host()
    np.testing.assert_array_equal(got.correlation, want.correlation)
    np.testing.assert_array_equal(got.autocorrelation, want.autocorrelation)
    _check_close(got, _fp64_fields(mov, pmd, "max", 3))


@pytest.mark.parametrize("mode", ["max", "mean"])
def test_agrees_with_existing_routines_dead_pixels(gpu_ctx, case, mode):
    """The four images agree with the existing routines on the same movie and the dense expansion; constant pixels
    give NaN / inf at the same positions (Python's max semantics of diagnostic_plots.py, kept by pmd_neighbour_image)."""
    mov, pmds = case
    pmd = pmds["F"]
    mov = mov.copy()
    mov[:, 4, 6] = 900.0
    mov[:, 0, 0] = 5.0
    mov[:, D1 - 1, D2 - 1] = 0.0
    dense = np.asarray(pmd[:, :, :], dtype=np.float32)
    got = localmd_amd.make_pmd_diagnostic_images(mov, pmd, mode=mode, lag=3, frame_batch_size=1024, ctx=gpu_ctx)
    want = (DI.make_correlation_image(mov, mode=mode, ctx=gpu_ctx), DI.make_autocorrelation_image(mov, lag=3, ctx=gpu_ctx),
            DI.make_pmd_correlation_image(mov, dense, mode=mode, ctx=gpu_ctx),
            DI.make_residual_correlation_image(mov, dense, mode=mode, ctx=gpu_ctx))
    for name, g, w, rtol in zip(DI.PMDDiagnostics._fields, got, want, (1e-5, 1e-5, 1e-4, 1e-3)):
        assert not np.isfinite(w).all(), name      # NaN (0 / 0) or, for the pmd image, inf (cov / 0)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=name)
        np.testing.assert_array_equal(np.isinf(g), np.isinf(w), err_msg=name)
        np.testing.assert_allclose(g, w, rtol=rtol, atol=1e-5, err_msg=name)
    dead = np.zeros((D1, D2), bool)
    dead[4, 6] = dead[0, 0] = dead[D1 - 1, D2 - 1] = True
    np.testing.assert_array_equal(np.isnan(got.explained_variance), dead)


def test_batch_size_invariance(gpu_ctx, case):
    mov, pmds = case
    pmd = pmds["F"]
    runs = [localmd_amd.make_pmd_diagnostic_images(mov, pmd, lag=3, frame_batch_size=b, ctx=gpu_ctx)
            for b in (1024, 2048, 4096, 10 ** 6)]
    for r in runs[1:]:
        np.testing.assert_array_equal(r.correlation, runs[0].correlation)
        np.testing.assert_array_equal(r.autocorrelation, runs[0].autocorrelation)
        _check_close(r, runs[0])


def test_source_invariance(gpu_ctx, case, tmp_path):
    import torch

    mov, pmds = case
    pmd = pmds["F"]
    u16 = mov.astype(np.uint16)
    assert np.array_equal(u16.astype(np.float32), mov)
    path = os.path.join(str(tmp_path), "movie.tif")
    write_tiff(path, u16)
    sources = {"u16": u16, "tiff": TiffArray(path), "cpu_tensor": torch.from_numpy(mov),
               "device_tensor": torch.from_numpy(mov).to(gpu_ctx.device)}
    want = localmd_amd.make_pmd_diagnostic_images(mov, pmd, lag=3, frame_batch_size=1024, ctx=gpu_ctx)
    for name, src in sources.items():
        got = localmd_amd.make_pmd_diagnostic_images(src, pmd, lag=3, frame_batch_size=1024, ctx=gpu_ctx)
        _assert_same(got, want)


class _CountingU16(lazy_data_loader):
    """Lazy uint16 movie generated on the fly (a fixed rank-6 model plus a bank of noise frames); counts how often every
    frame is served."""

    def __init__(self, n, d1, d2):
        rng = np.random.default_rng(5)
        self._shape = (n, d1, d2)
        yy, xx = np.mgrid[0:d1, 0:d2]
        cy, cx = rng.uniform(0, d1, 6), rng.uniform(0, d2, 6)
        self.space = np.stack([np.exp(-((yy - a) ** 2 + (xx - b) ** 2) / 60.0).reshape(-1) for a, b in zip(cy, cx)])
        self.space = self.space.astype(np.float32)
        self.freq = rng.uniform(0.001, 0.02, 6)
        self.noise = rng.normal(0, 8.0, (64, d1 * d2)).astype(np.float32)
        self.count = np.zeros(n, dtype=np.int64)

    @property
    def dtype(self):
        return np.uint16

    @property
    def shape(self):
        return self._shape

    def _compute_at_indices(self, indices):
        idx = np.arange(self._shape[0])[indices].reshape(-1)
        np.add.at(self.count, idx, 1)
        tr = 400.0 * (1.0 + np.sin(idx[:, None] * self.freq[None, :] * 2 * np.pi))
        fr = tr.astype(np.float32) @ self.space + 1000.0 + self.noise[(idx * 7919) % 64]
        return np.clip(np.round(fr), 0, 65535).astype(np.uint16).reshape(len(idx), *self._shape[1:])


def test_long_movie_read_once_bounded_memory(gpu_ctx):
    import torch

    n, d1, d2 = 20000, 128, 128
    src = _CountingU16(n, d1, d2)
    np.random.seed(1)
    pmd = localmd_amd.localmd_decomposition(src, (32, 32), 2000, max_components=6, background_rank=2, seed=5, sim_iters=5,
                                            ctx=gpu_ctx)
    src.count[:] = 0
    gpu_ctx.release_workspace()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    got = localmd_amd.make_pmd_diagnostic_images(src, pmd, lag=2, frame_batch_size=1024, ctx=gpu_ctx)
    peak = torch.cuda.max_memory_allocated()
    assert peak < 0.25 * 4 * n * d1 * d2, peak / 1e9
    assert np.all(src.count == 1), np.unique(src.count)
    assert got.frame_residual_rms.shape == (n,)
    for name, f in zip(DI.PMDDiagnostics._fields, got):
        assert np.all(np.isfinite(f)), name
    # the model is rank 6 with local footprints plus noise of std 8: the residual is about the noise, and the
    # decomposition explains most of the variance where the footprints are bright
    assert 6.0 < np.median(got.residual_std) < 9.0
    assert 6.0 < np.median(got.frame_residual_rms) < 9.0
    assert np.max(got.explained_variance) > 0.5
