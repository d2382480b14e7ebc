"""
Host-side planning of the streamed decomposition (stream=True): frame batches, the gather maps of the fit frames and
the background sample, the auto-mode decision and the argument checks, and the staged upload on a CPU device.  No
device needed.
"""
import json
import os
import re

import numpy as np
import pytest

from localmd_amd import _movie as Mv
from localmd_amd import decomposition as Dm
from localmd_amd import grid
from localmd_amd.dataset import ArrayDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("T", [1000, 1024, 5000, 10001])
@pytest.mark.parametrize("batch", [1000, 1024, 10000])
def test_batches_fall_on_chunk_boundaries(T, batch):
    b = Mv._stream_batches(T, batch)
    assert b[0][0] == 0 and b[-1][1] == T
    for (a0, a1), (c0, _) in zip(b, b[1:]):
        assert a1 == c0
    for t0, t1 in b:
        assert t0 % 1024 == 0 and t1 > t0
    for t0, t1 in b[:-1]:
        assert (t1 - t0) % 1024 == 0
    nb = Mv._stream_batch_frames(batch)
    assert nb == max(1024, batch // 1024 * 1024)
    assert all(t1 - t0 <= nb for t0, t1 in b)


@pytest.mark.parametrize("T,frame_range,window,batch", [(10001, 3000, 500, 1024), (5000, 2500, 1000, 1000),
                                                        (20000, 4000, 700, 3000), (3000, 3000, 3000, 1024)])
def test_gather_maps_cover_every_requested_frame_once(T, frame_range, window, batch):
    np.random.seed(3)
    sample = np.random.choice(list(range(T)), replace=False, size=min(1000, T)).tolist()
    frames = grid.identify_window_chunks(frame_range, T, window)
    batches = Mv._stream_batches(T, batch)
    for lst in (frames, sample):
        maps = Mv._gather_maps(lst, batches)
        assert len(maps) == len(batches)
        seen = np.zeros(len(lst), dtype=np.int64)
        for (t0, t1), (src, dst) in zip(batches, maps):
            assert src.dtype == np.int32 and dst.dtype == np.int32 and len(src) == len(dst)
            assert np.all((src >= 0) & (src < t1 - t0))
            np.testing.assert_array_equal(np.asarray(lst)[dst], src + t0)
            seen[dst] += 1
        assert np.all(seen == 1)


def _baseline_shapes():
    cfg = json.load(open(os.path.join(ROOT, "BASELINE.json")))["configs"]
    shapes = []
    for c in cfg:
        m = re.search(r"(\d+)×(\d+)×(\d+)", c if isinstance(c, str) else json.dumps(c, ensure_ascii=False))
        if m:
            shapes.append(tuple(int(x) for x in m.groups()))
    return shapes


def test_auto_mode_keeps_every_baseline_config_resident():
    shapes = _baseline_shapes()
    assert len(shapes) >= 4
    free = 288e9
    for d1, d2, T in shapes:
        assert Mv._plan_mode(None, T, d1 * d2, free) == "resident", (d1, d2, T)
        assert Mv._plan_mode(False, T, d1 * d2, free) == "resident"
        assert Mv._plan_mode(True, T, d1 * d2, free) == "stream"
    # a movie larger than the free memory streams; one that cannot be streamed stays resident (and fails there)
    T, D = 100_000, 512 * 512           # 105 GB of fp32
    assert Mv._plan_mode(None, T, D, 100e9) == "stream"
    assert Mv._plan_mode(None, T, D, 100e9, streamable=False) == "resident"


def test_stream_dtype_and_sources():
    assert Mv._stream_dtype(np.zeros((2, 3, 3), np.uint16)) == np.uint16
    assert Mv._stream_dtype(ArrayDataset(np.zeros((2, 3, 3), np.int16))) == np.int16
    assert Mv._stream_dtype(np.zeros((2, 3, 3), np.float64)) == np.float32
    assert Mv._stream_dtype(np.zeros((2, 3, 3), np.uint8)) == np.float32
    assert Mv._stream_source_problem(np.zeros((2, 3, 3)), False) is None
    assert Mv._stream_source_problem(ArrayDataset(np.zeros((2, 3, 3))), False) is None


class _SlabSource:
    shape = (300, 20, 20)
    dtype = np.float32

    def slab(self, lo, hi):
        raise AssertionError("not reached")


def test_stream_true_rejects_unsupported_sources():
    import torch

    mov = np.zeros((300, 20, 20), dtype=np.float32)
    with pytest.raises(ValueError, match="distributed"):
        Dm.localmd_decomposition(mov, (10, 10), 300, stream=True, distributed=True)
    with pytest.raises(ValueError, match="slab"):
        Dm.localmd_decomposition(_SlabSource(), (10, 10), 300, stream=True)
    dev_tensor = torch.empty((300, 20, 20), dtype=torch.float32, device="meta")
    with pytest.raises(ValueError, match="device tensor"):
        Dm.localmd_decomposition(dev_tensor, (10, 10), 300, stream=True)
    # a CPU tensor is a host source
    assert Mv._stream_source_problem(torch.zeros((3, 4, 4)), False) is None


def test_auto_mode_counts_the_allocator_cache_as_free():
    """After a large call the caching allocator keeps its blocks reserved: the driver then reports little free memory,
    but the resident path would reuse those blocks.  Auto mode must decide on driver-free + reserved-but-unused."""
    GB = 1e9
    # BASELINE config 4 left ~251 GB reserved (nothing allocated); the driver reports ~37 GB free of 288
    usable = Mv._usable_free_bytes(37 * GB, 251 * GB, 0)
    assert usable == 288 * GB
    T, D = 30000, 250_000                      # a 30 GB fp32 movie
    assert Mv._plan_mode(None, T, D, 37 * GB) == "stream"          # what the driver figure alone would decide
    assert Mv._plan_mode(None, T, D, usable) == "resident"
    # live tensors are not free: only the reserved-but-unallocated part counts
    assert Mv._usable_free_bytes(37 * GB, 251 * GB, 200 * GB) == 88 * GB
    assert Mv._usable_free_bytes(37 * GB, 10 * GB, 10 * GB) == 37 * GB


def test_fit_estimate_counts_the_tile_stage():
    """Small blocks over a large field of view: the per-tile traces outweigh the fit frames, and the estimate that turns
    a device out-of-memory error into a ValueError must include them (up to one tile batch)."""
    D, rows, n_fit = 1024 * 1024, 1024 * 1024 + 1024, 5000
    ld_fit, ld_proj = 5000 // 64 * 64 + 128, 2048 + 64
    n_tiles = 203 * 203                        # 10 x 10 blocks at 50 % overlap
    small = Dm._stream_tile_bytes(n_tiles, 64, 128, ld_fit, ld_proj, 24 << 30)
    assert small > 24 << 30                    # one batch of traces plus U and U W of every tile
    assert Dm._stream_tile_bytes(n_tiles, 64, 128, ld_fit, ld_proj, 1 << 50) > 3 * 4 * rows * ld_fit
    base = Mv._stream_fit_bytes(2, D, rows, ld_fit, n_fit, 1000, 9216, 0)
    assert Mv._stream_fit_bytes(2, D, rows, ld_fit, n_fit, 1000, 9216, small) == base + small


_RING_D1, _RING_D2 = 5, 7


def _ring_batches(monkeypatch, src, data, staged, rows=None):
    """The batches of _stream_batches(T, 1024) through one _StagingRing on a CPU device, 300 frames a piece, into two
    alternating (1024, D) destinations: after each call the destination rows are the frames of the batch, exactly."""
    import types
    import torch

    T = len(data)
    i_lo, i_hi = (0, _RING_D1) if rows is None else rows
    D = (i_hi - i_lo) * _RING_D2
    monkeypatch.setattr(Mv._StagingRing, "STAGE_BYTES", 300 * D * np.dtype(staged).itemsize)
    fake_ctx = types.SimpleNamespace(device=torch.device("cpu"))
    tdtype = torch.from_numpy(np.zeros(1, dtype=staged)).dtype
    dst = [torch.zeros((1024, D), dtype=tdtype) for _ in range(2)]
    batches = Mv._stream_batches(T, 1024)
    assert all(b0 > 0 for b0, _ in batches[1:])
    with Mv._StagingRing(fake_ctx, src, tdtype, 1024, rows=rows) as ring:
        assert ring.step == 300
        for k, (b0, b1) in enumerate(batches):
            assert ring.upload(dst[k % 2], b0, b1) is None           # a CPU device: synchronous copies, no event
            got = dst[k % 2][:b1 - b0].numpy()
            assert got.dtype == np.dtype(staged)
            np.testing.assert_array_equal(got, data[b0:b1, i_lo:i_hi, :].astype(staged).reshape(b1 - b0, D))
            assert len(ring.stage) == Mv._StagingRing.STAGE_BUFFERS
            assert len(Mv._StagingRing._stage_cache) == 1


@pytest.mark.parametrize("T", [1, 1023, 1025, 2049, 3073])
@pytest.mark.parametrize("lazy", [False, True], ids=["array", "loader"])
@pytest.mark.parametrize("dtype,staged", [(np.float32, np.float32), (np.uint16, np.uint16), (np.int16, np.int16),
                                          (np.float64, np.float32)])
def test_staging_ring_uploads_batches_on_a_cpu_device(monkeypatch, T, lazy, dtype, staged):
    """The staged upload of the streamed passes without a GPU.  T = 1025 leaves a batch of exactly one frame (a
    lazy_data_loader returns it 2-D); uint16 / int16 travel as they are, float64 is staged as float32."""
    rng = np.random.default_rng(T)
    data = (rng.random((T, _RING_D1, _RING_D2)) * 2000 - (1000 if np.dtype(dtype).kind != "u" else 0)).astype(dtype)
    src = ArrayDataset(data) if lazy else data
    assert Mv._stream_dtype(src) == np.dtype(staged)
    _ring_batches(monkeypatch, src, data, staged)
    if T == 2049:
        _ring_batches(monkeypatch, src, data, staged, rows=(1, 4))     # a FOV row band: the cropped frames
