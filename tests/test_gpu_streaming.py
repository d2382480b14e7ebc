"""
Streamed decomposition (stream=True) on the device: the batch kernels against their whole-movie counterparts bit for
bit, the streamed pipeline against the resident one under the same seeds, and a movie far larger than what the
streamed mode keeps on the device, read exactly twice.
"""
import os

import numpy as np
import pytest

from tests import parity_metrics as PM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELEM = {np.dtype(np.float32): 0, np.dtype(np.uint16): 1, np.dtype(np.int16): 2}


def _t():
    import torch

    return torch


def P(t):
    from localmd_amd._lib import ptr

    return ptr(t)


def dev(ctx, a):
    return _t().from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _movie(T, d1, d2, seed=1):
    from localmd_amd.synthetic import make_movie

    return make_movie(T, d1, d2, seed=seed)


def _typed(mov, dtype):
    """Integer version of a synthetic movie (exactly representable in fp32)."""
    if dtype == np.uint16:
        return np.clip(np.round(mov * 40.0 + 2000.0), 0, 65535).astype(np.uint16)
    if dtype == np.int16:
        return np.clip(np.round(mov * 40.0 - 300.0), -32768, 32767).astype(np.int16)
    return mov.astype(np.float32)


def _whole_stats(ctx, mov32, cn):
    torch = _t()
    T, D = mov32.shape
    mean = torch.empty(D, dtype=torch.float32, device=ctx.device)
    std = torch.empty(D, dtype=torch.float32, device=ctx.device)
    ws = torch.empty(ctx.lib.pmd_stats_workspace_bytes(T, D, 1024), dtype=torch.uint8, device=ctx.device)
    md = dev(ctx, mov32)
    ctx.call("pmd_stats", P(md), T, D, 1024, cn, P(mean), P(std), P(ws), ws.numel())
    return mean.cpu().numpy(), std.cpu().numpy()


def _streamed_stats(ctx, mov, batch, cn):
    torch = _t()
    T, D = mov.shape
    mean = torch.empty(D, dtype=torch.float32, device=ctx.device)
    std = torch.empty(D, dtype=torch.float32, device=ctx.device)
    ws = torch.empty(ctx.lib.pmd_stats_stream_workspace_bytes(T, D), dtype=torch.uint8, device=ctx.device)
    # batches handed over in reverse order: the partials land at their chunk, whatever the order of the calls
    for t0 in reversed(range(0, T, batch)):
        n = min(batch, T - t0)
        b = dev(ctx, mov[t0:t0 + n])
        ctx.call("pmd_stats_stream_accumulate", P(b), ELEM[mov.dtype], t0, n, T, D, cn, P(ws), ws.numel())
    ctx.call("pmd_stats_stream_finish", T, D, cn, P(mean), P(std), P(ws), ws.numel())
    return mean.cpu().numpy(), std.cpu().numpy()


@pytest.mark.parametrize("T,compute_normalizer", [(2100, True), (1300, True), (200, True), (700, False)])
@pytest.mark.parametrize("dtype", [np.float32, np.uint16, np.int16])
def test_streamed_stats_equal_pmd_stats_bit_for_bit(gpu_ctx, T, compute_normalizer, dtype):
    d1, d2 = 23, 31
    mov = _typed(_movie(T, d1, d2, seed=3).reshape(T, d1 * d2), dtype)
    cn = 1 if compute_normalizer else 0
    ref_mean, ref_std = _whole_stats(gpu_ctx, mov.astype(np.float32), cn)
    for batch in (1024, 3072):     # 2100 frames in 1024-batches: a ragged last batch of 52 frames
        mean, std = _streamed_stats(gpu_ctx, mov, batch, cn)
        np.testing.assert_array_equal(mean, ref_mean)
        np.testing.assert_array_equal(std, ref_std)
    if compute_normalizer and T >= 256:
        assert np.all(ref_std != 1.0)


def test_streamed_stats_reject_misaligned_batches(gpu_ctx):
    from localmd_amd._lib import PMDLibraryError

    torch = _t()
    T, D = 3000, 64
    ws = torch.empty(gpu_ctx.lib.pmd_stats_stream_workspace_bytes(T, D), dtype=torch.uint8, device=gpu_ctx.device)
    b = torch.zeros((1500, D), dtype=torch.float32, device=gpu_ctx.device)
    for t0, n in ((512, 1024), (0, 1500)):      # not on a chunk boundary / a split chunk that is not the last
        with pytest.raises(PMDLibraryError):
            gpu_ctx.call("pmd_stats_stream_accumulate", P(b), 0, t0, n, T, D, 1, P(ws), ws.numel())


@pytest.mark.parametrize("dtype", [np.uint16, np.int16])
def test_typed_standardize_transpose_equals_fp32_kernel(gpu_ctx, dtype):
    torch = _t()
    ctx = gpu_ctx
    T, d1, d2 = 300, 20, 18
    D = d1 * d2
    mov = _typed(_movie(T, d1, d2, seed=4).reshape(T, D), dtype)
    m32 = mov.astype(np.float32)
    mean = dev(ctx, m32.mean(axis=0).astype(np.float32))
    std = dev(ctx, (m32.std(axis=0) + 0.5).astype(np.float32))
    rng = np.random.default_rng(0)
    for frames in (None, rng.choice(T, size=121, replace=False).astype(np.int32)):
        nf = T if frames is None else len(frames)
        ld = ctx.lib.pmd_time_ld(nf)
        fr = None if frames is None else dev(ctx, frames)
        outs = []
        for src, elem in ((dev(ctx, m32), 0), (dev(ctx, mov), ELEM[np.dtype(dtype)])):
            out = torch.full((1024, ld), 7.0, dtype=torch.float32, device=ctx.device)
            ctx.call("pmd_standardize_transpose_typed", P(src), elem, D, P(fr), nf, P(mean), P(std), P(out), ld)
            outs.append(out.cpu().numpy())
        ref = torch.full((1024, ld), 7.0, dtype=torch.float32, device=ctx.device)
        m32_d = dev(ctx, m32)
        ctx.call("pmd_standardize_transpose", P(m32_d), D, P(fr), nf, P(mean), P(std), P(ref), ld)
        ref = ref.cpu().numpy()
        np.testing.assert_array_equal(outs[0], ref)
        np.testing.assert_array_equal(outs[1], ref)
        assert np.all(ref[:D, nf:ld] == 0)        # zero columns up to ld
        assert np.all(ref[D:] == 7.0)             # rows beyond D untouched


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_gather_frames(gpu_ctx, dtype):
    torch = _t()
    ctx = gpu_ctx
    n, D = 200, 1000
    src = _typed(_movie(n, 20, 50, seed=2).reshape(n, D), dtype)
    src_rows = np.array([5, 0, 199, 37, 38], dtype=np.int32)
    dst_rows = np.array([4, 2, 0, 1, 3], dtype=np.int32)
    src_d, sr_d, dr_d = dev(ctx, src), dev(ctx, src_rows), dev(ctx, dst_rows)   # (alive across the call)
    out = torch.zeros((6, D), dtype=src_d.dtype, device=ctx.device)
    ctx.call("pmd_gather_frames", P(src_d), ELEM[np.dtype(dtype)], D, P(sr_d), P(dr_d), len(src_rows), P(out))
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[dst_rows], src[src_rows])
    assert np.all(got[5] == 0)


# ---- pipeline: stream=True against stream=False -------------------------------------------------------------------

def _run(gpu_ctx, mov, blk, frames, **kw):
    import localmd_amd

    np.random.seed(7)
    return localmd_amd.localmd_decomposition(mov, blk, frames, seed=11, sim_iters=8, return_diagnostics=True, ctx=gpu_ctx,
                                             **kw)


def _check_same(a, da, b, db, shape):
    assert db["streamed"] and not da["streamed"]
    assert db["stream_bytes_uploaded"] > 0
    assert "stream_stats" in db["timings"] and "stream_projection" in db["timings"]
    np.testing.assert_array_equal(b.mean_img, a.mean_img)
    np.testing.assert_array_equal(b.var_img, a.var_img)
    assert db["frames"] == da["frames"]
    np.testing.assert_array_equal(db["tile_ranks"], da["tile_ranks"])
    np.testing.assert_array_equal(db["tile_ut"], da["tile_ut"])
    np.testing.assert_array_equal(b.u.indices, a.u.indices)
    np.testing.assert_array_equal(b.u.indptr, a.u.indptr)
    np.testing.assert_array_equal(b.u.data, a.u.data)
    assert b.s.shape == a.s.shape
    tol = np.maximum(2e-5, 2e-6 * (a.s[0] / a.s) ** 2)
    strong = a.s > 1e-2 * a.s[0]
    assert np.all((np.abs(b.s - a.s) / a.s)[strong] <= tol[strong]), np.max((np.abs(b.s - a.s) / a.s / tol)[strong])
    assert PM.probes(b, a, shape, n=400) < 2e-4


def _compare(gpu_ctx, mov, blk, frames, **kw):
    from localmd_amd import decomposition as Dm

    Dm.QUIET = True
    a, da = _run(gpu_ctx, mov, blk, frames, stream=False, **kw)
    b, db = _run(gpu_ctx, mov, blk, frames, stream=True, frame_batch_size=1024, **kw)
    _check_same(a, da, b, db, tuple(int(x) for x in mov.shape))
    return da, db


def test_stream_matches_resident_on_the_memory_plan_movies(gpu_ctx):
    """The two movies / blocks of the tile-batch and single-copy test (both routes of the global stage), all frames
    fitted; and with tile batches."""
    routes = set()
    for mov, blk, kw in [(_movie(500, 60, 70, seed=4), (20, 20), dict(max_components=6, background_rank=3)),
                         (_movie(300, 70, 80, seed=3), (10, 10), dict(max_components=8, background_rank=3))]:
        da, _ = _compare(gpu_ctx, mov, blk, mov.shape[0], **kw)
        routes.add(da["orthogonalizer"])
        _compare(gpu_ctx, mov, blk, mov.shape[0], tile_batch_bytes=1, **kw)
    assert routes == {"cholesky", "eigh"}, routes


@pytest.mark.parametrize("case", [
    dict(frames=600),                                            # frame_range < T, several batches
    dict(frames=2500),                                           # frame_range = T
    dict(frames=600, window_chunks=200),                         # three windows
    dict(frames=600, background_rank=0),
    dict(frames=600, pixel_weighting="ramp"),
    dict(frames=600, tile_batch_bytes=1),
])
def test_stream_matches_resident(gpu_ctx, case):
    case = dict(case)
    mov = _movie(2500, 40, 50, seed=6)
    if case.get("pixel_weighting") == "ramp":
        case["pixel_weighting"] = np.linspace(0.5, 1.5, 40 * 50, dtype=np.float32).reshape(40, 50)
    kw = dict(max_components=6, background_rank=3)
    kw.update({k: v for k, v in case.items() if k != "frames"})
    _compare(gpu_ctx, mov, (20, 20), case["frames"], **kw)


def test_stream_matches_resident_uint16_sources(gpu_ctx):
    from localmd_amd.dataset import ArrayDataset, TiffArray

    mov16 = _typed(_movie(2300, 40, 40, seed=8), np.uint16)
    _compare(gpu_ctx, ArrayDataset(mov16), (20, 20), 700, max_components=5, background_rank=2)
    tif = TiffArray(os.path.join(ROOT, "tests", "golden", "pillow_u16_lzw.tif"))
    _compare(gpu_ctx, tif, (20, 26), tif.shape[0], max_components=2, background_rank=1, temporal_avg_factor=4)


class _CountingLowRank:
    """Lazy uint16 movie generated on the fly: a fixed rank-6 model plus a bank of noise frames, so the host holds one
    batch at a time.  Counts how often every frame is served."""

    def __init__(self, T, d1, d2):
        rng = np.random.default_rng(5)
        self.shape = (T, d1, d2)
        self.dtype = np.uint16
        yy, xx = np.mgrid[0:d1, 0:d2]
        cy, cx = rng.uniform(0, d1, 6), rng.uniform(0, d2, 6)
        self.space = np.stack([np.exp(-((yy - a) ** 2 + (xx - b) ** 2) / 60.0).reshape(-1) for a, b in zip(cy, cx)])
        self.freq = rng.uniform(0.001, 0.02, 6)
        self.noise = rng.normal(0, 8.0, (64, d1 * d2)).astype(np.float32)
        self.count = np.zeros(T, dtype=np.int64)

    def __getitem__(self, key):
        idx = np.asarray(key, dtype=np.int64).reshape(-1)
        np.add.at(self.count, idx, 1)
        tr = 400.0 * (1.0 + np.sin(idx[:, None] * self.freq[None, :] * 2 * np.pi))
        fr = tr.astype(np.float32) @ self.space.astype(np.float32) + 1000.0 + self.noise[(idx * 7919) % 64]
        return np.clip(np.round(fr), 0, 65535).astype(np.uint16).reshape(len(idx), *self.shape[1:]).squeeze()


def test_stream_bounded_memory_two_passes(gpu_ctx):
    import localmd_amd
    from localmd_amd import decomposition as Dm

    torch = _t()
    Dm.QUIET = True
    T, d1, d2 = 40000, 256, 256
    src = _CountingLowRank(T, d1, d2)
    kw = dict(max_components=6, background_rank=3, seed=11, sim_iters=8, return_diagnostics=True, ctx=gpu_ctx)
    gpu_ctx.release_workspace()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    np.random.seed(2)
    b, db = localmd_amd.localmd_decomposition(src, (32, 32), 2000, stream=True, **kw)
    peak = torch.cuda.max_memory_allocated()
    assert peak < 0.5 * 4 * T * d1 * d2, peak / 1e9
    assert np.all(src.count == 2), np.unique(src.count)
    assert db["streamed"] and db["stream_bytes_uploaded"] == 2 * 2 * T * d1 * d2
    assert np.all(np.isfinite(b.s)) and np.all(np.isfinite(b.v)) and np.all(np.isfinite(b.r))
    gpu_ctx.release_workspace()
    np.random.seed(2)
    a, da = localmd_amd.localmd_decomposition(src, (32, 32), 2000, stream=False, **kw)
    assert not da["streamed"]
    np.testing.assert_array_equal(db["tile_ranks"], da["tile_ranks"])
    np.testing.assert_array_equal(b.u.indices, a.u.indices)
    np.testing.assert_array_equal(b.u.indptr, a.u.indptr)
    assert b.s.shape == a.s.shape
    gpu_ctx.release_workspace()
