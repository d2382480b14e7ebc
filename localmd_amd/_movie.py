"""
The movie sources of the Python side, the layer below the decomposition driver (decomposition.py) and the movie-pass
scaffold of the PMDArray consumers (_stream.py): the movie resident in HBM (_Movie) or left at its host source and read
in frame batches (_StreamedMovie), the staged upload both go through (_StagingRing: reader threads, a kept ring of
page-locked buffers, asynchronous copies on a side stream), the frame-batch plan, the element-type table of the typed
kernels and the free-memory query.  PyTorch is used for device memory, streams and copies only, and imported lazily.
"""
import concurrent.futures
import os

import numpy as np

from ._lib import ptr, C


def _torch():
    # every allocation looks `empty` / `zeros` up on the module at call time (torch = _torch(); never `from torch import
    # empty`): the poison tests replace torch.empty, and code that bypasses the attribute silently leaves them
    import torch

    return torch


def _upload(ctx, arr, np_dtype):
    """Host table -> device tensor.  Large tables go through a page-locked staging buffer of the context and an
    asynchronous copy (released with ctx.release_pinned() after the next synchronisation)."""
    torch = _torch()
    a = np.ascontiguousarray(arr, dtype=np_dtype)
    t = torch.from_numpy(a)
    if a.nbytes < (1 << 18) or not hasattr(ctx, "pinned") or ctx.device.type != "cuda":
        return t.to(ctx.device)
    stage = ctx.pinned(a.nbytes)[:a.nbytes].view(t.dtype).view(t.shape)
    stage.copy_(t)
    return stage.to(ctx.device, non_blocking=True)


def _i32(ctx, arr):
    return _upload(ctx, arr, np.int32)


def _f32(ctx, arr):
    return _upload(ctx, arr, np.float32)


def _round_up(x, m):
    return (x + m - 1) // m * m


_SIDE_STREAMS = {}


def _side_stream(device):
    """One extra HIP stream per device for result downloads that overlap compute."""
    torch = _torch()
    key = str(device)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[key]


_ELEM = {np.dtype(np.float32): 0, np.dtype(np.uint16): 1, np.dtype(np.int16): 2}   # PMD_ELEM_F32 / _U16 / _I16


def _device_elem(t):
    """_ELEM code of a tensor's element type, None for a type the kernels do not read."""
    torch = _torch()
    m = {torch.float32: 0, torch.int16: 2}
    if hasattr(torch, "uint16"):
        m[torch.uint16] = 1
    return m.get(t.dtype)


def _reader_threads(dataset_obj, is_array, num_workers):
    # num_workers = 0 is in-process, single-threaded loading in the reference (pmd_loader.py:161-168; workers > 0 are
    # separate processes with a dataset copy each).  A user's lazy_data_loader may share a file handle or a decoder
    # that is not re-entrant, so its __getitem__ is called from ONE reader thread unless num_workers > 0 is passed,
    # which then promises a thread-safe __getitem__ (as does a true `thread_safe` attribute of the loader, which the
    # built-in TiffArray has).  Slicing a NumPy array is thread-safe: many copy threads.
    if num_workers and num_workers > 0:
        return int(num_workers)
    return min(32, os.cpu_count() or 1) if (is_array or getattr(dataset_obj, "thread_safe", False)) else 1


class _StagingRing:
    """Host -> HBM ingestion (reference: FrameDataloader + torch DataLoader workers, pmd_loader.py:71-108,
    :151-168, reading a lazy_data_loader such as TiffArray, dataset.py:131-181).  Pieces of at most `max_frames` frames
    and STAGE_BYTES bytes are read / decoded by worker threads straight into page-locked staging buffers of `dtype` (a
    ring of STAGE_BUFFERS) and leave by asynchronous DMA on a copy stream, so decoding piece k + 1 overlaps the transfer
    of piece k; a buffer is reused once the event recorded behind its transfer has completed.  rows = (i_lo, i_hi):
    only these FOV rows (first spatial axis) are uploaded.  On a CPU device the ring is pageable and the copies are
    synchronous.  A context: left with the pool shut down and the main stream waiting for the uploads."""

    STAGE_BUFFERS = 3
    STAGE_BYTES = 64 << 20
    _stage_cache = {}     # (frames per buffer, D, pinned, dtype) -> ring of staging buffers, kept between calls (page-locking is slow)

    def __init__(self, ctx, src, dtype, max_frames, num_workers=0, rows=None):
        torch = _torch()
        self.src, self.is_array = src, isinstance(src, np.ndarray)
        self.frame = tuple(int(x) for x in src.shape[1:])
        self.rows = slice(0, self.frame[0]) if rows is None else slice(*rows)
        D = (self.rows.stop - self.rows.start) * self.frame[1]
        on_gpu = ctx.device.type == "cuda"
        self.step = max(1, min(int(max_frames), self.STAGE_BYTES // max(dtype.itemsize * D, 1)))
        self.n_threads = _reader_threads(src, self.is_array, num_workers)
        key = (self.step, D, on_gpu, dtype)
        if key not in self._stage_cache:
            self._stage_cache.clear()
            self._stage_cache[key] = [torch.empty((self.step, D), dtype=dtype, pin_memory=on_gpu) for _ in range(self.STAGE_BUFFERS)]
        self.stage = self._stage_cache[key]
        self.stage_np = [b.numpy() for b in self.stage]
        self.done = [None] * len(self.stage)     # event behind the transfer that last read a staging buffer
        self.k = 0                               # pieces so far: piece k goes through buffer k % len(stage)
        self.main = torch.cuda.current_stream(ctx.device) if on_gpu else None
        self.copy_stream = _side_stream(ctx.device) if on_gpu else None
        if on_gpu:
            self.copy_stream.synchronize()            # the staging ring is kept between calls: no transfer of an earlier call may still read it
            self.copy_stream.wait_stream(self.main)   # the destination may reuse a block still in use on the main stream
        self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=self.n_threads)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.pool.shutdown()
        if exc_type is None and self.copy_stream is not None:
            self.main.wait_stream(self.copy_stream)

    def _fill(self, buf, t0, t1, base):
        """frames [t0, t1) -> rows [t0 - base, t1 - base) of staging buffer `buf` (runs on a worker thread)."""
        # lazy_data_loader.__getitem__ ends with .squeeze() (dataset.py:114): a one-frame batch comes back 2-D
        part = self.src[t0:t1] if self.is_array else np.asarray(self.src[list(range(t0, t1))]).reshape((t1 - t0,) + self.frame)
        part = part[:, self.rows, :]
        np.copyto(self.stage_np[buf][t0 - base:t1 - base].reshape(part.shape), part, casting="unsafe")

    def upload(self, dst, b0, b1):
        """Frames [b0, b1) of the source -> rows [0, b1 - b0) of the (frames, D) tensor `dst`, piece by piece.  Returns
        the event recorded behind the last piece's transfer (the copies are in order), None on a CPU device."""
        torch = _torch()
        submit, fill = self.pool.submit, self._fill
        for base in range(b0, b1, self.step):
            n = min(self.step, b1 - base)
            buf = self.k % len(self.stage)
            self.k += 1
            if self.done[buf] is not None:
                self.done[buf].synchronize()     # the transfer that last read this buffer has finished
            parts = max(1, min(self.n_threads, n))
            edges = [base + (n * p) // parts for p in range(parts + 1)]
            for f in [submit(fill, buf, edges[p], edges[p + 1], base) for p in range(parts)]:
                f.result()
            if self.copy_stream is None:
                dst[base - b0:base - b0 + n].copy_(self.stage[buf][:n])
                continue
            with torch.cuda.stream(self.copy_stream):
                dst[base - b0:base - b0 + n].copy_(self.stage[buf][:n], non_blocking=True)
                self.done[buf] = torch.cuda.Event()
                self.done[buf].record(self.copy_stream)
        return self.done[(self.k - 1) % len(self.stage)]


class _Movie:
    """The (T, D) float32 movie resident in HBM, plus the pixel-major standardised copies."""

    def __init__(self, ctx, dataset_obj, frame_batch_size, rows=None, num_workers=0):
        """rows = (i_lo, i_hi): keep only these FOV rows (first spatial axis) - the pixel slab of one rank.
        self.D is the number of resident pixels; pixel c of the slab is FOV pixel c + i_lo * d2 (C order)."""
        torch = _torch()
        self.ctx = ctx
        shape = tuple(int(x) for x in dataset_obj.shape)
        self.T, self.d1, self.d2 = shape
        i_lo, i_hi = (0, self.d1) if rows is None else rows
        self.D = (i_hi - i_lo) * self.d2
        self.owned = True    # False: self.dev aliases the caller's tensor (releasing it frees nothing)
        if hasattr(dataset_obj, "slab"):   # a source that can build a band of FOV rows on the device
            mv = dataset_obj.slab(i_lo, i_hi).to(device=ctx.device, dtype=torch.float32)
            self.dev = mv.reshape(self.T, self.D).contiguous()
        elif isinstance(dataset_obj, torch.Tensor):
            mv = dataset_obj[:, i_lo:i_hi, :].to(device=ctx.device, dtype=torch.float32)
            self.dev = mv.reshape(self.T, self.D).contiguous()
            self.owned = self.dev.data_ptr() != dataset_obj.data_ptr()
        else:
            self.dev = torch.empty((self.T, self.D), dtype=torch.float32, device=ctx.device)
            with _StagingRing(ctx, dataset_obj, torch.float32, min(int(frame_batch_size), self.T), num_workers,
                              rows=(i_lo, i_hi)) as ring:
                ring.upload(self.dev, 0, self.T)
        # one extra block of zero rows: kernels that walk the rows in 1024-blocks may start at any owned offset
        self.rows_alloc = _round_up(self.D, 1024) + 1024

    def release(self):
        """Drop the raw frames-first copy once every standardised copy has been written (statistics, the background
        sample and the standardised movies are its only readers): 1/3 of the resident bytes of a large movie."""
        self.dev = None

    # ---- what the driver asks of a movie: statistics, standardized, release (the same three on _StreamedMovie)
    streamed = False
    statistics_phase = "stats"      # key of the statistics pass in diag["timings"]
    bytes_uploaded = 0              # counted by the streamed passes only

    def statistics(self, compute_normalizer, mean, std, frames=None, sample=None):
        """Per-pixel mean and noise level of the resident frames (frames / sample are gathered later, by standardized)."""
        ctx = self.ctx
        ws = ctx.workspace(ctx.lib.pmd_stats_workspace_bytes(self.T, self.D, 1024))
        ctx.call("pmd_stats", ptr(self.dev), self.T, self.D, 1024, 1 if compute_normalizer else 0, ptr(mean), ptr(std),
                 ptr(ws), ws.numel())

    def standardized(self, which, mean, std, frames=None):
        """Pixel-major (rows_alloc x ld) standardised copy `which` ("sample", "fit" or "all") of the listed frames;
        frames=None means all, in order."""
        torch = _torch()
        ctx = self.ctx
        nf = self.T if frames is None else len(frames)
        ld = ctx.lib.pmd_time_ld(nf)
        # the kernel writes every column of the D pixel rows (zeros beyond nf); only the row padding needs a fill
        out = torch.empty((self.rows_alloc, ld), dtype=torch.float32, device=ctx.device)
        if self.rows_alloc > self.D:
            out[self.D:].zero_()
        fr = None if frames is None else _i32(ctx, frames)
        ctx.call("pmd_standardize_transpose", ptr(self.dev), self.D, ptr(fr), nf, ptr(mean), ptr(std), ptr(out), ld)
        return out, ld


# ---- streamed mode: movies longer than device memory (reference: lazy_data_loader / FrameDataloader batches,
# pmd_loader.py:71-108; statistics pass :203-291; projection pass :316-346).  Only the fit frames, the background
# sample, two frame batches, the per-pixel statistics and Z live on the device; the movie is read twice from its source.
STREAM_CHUNK = 1024          # frames per Welch chunk (PMD_STATS_CHUNK): batch boundaries fall on chunk boundaries
STREAM_PROJECT_FRAMES = 2048  # frames per standardise + project step of pass 2 (bounds its pixel-major scratch)


def _stream_batch_frames(frame_batch_size):
    """frame_batch_size rounded down to whole 1024-frame chunks, at least one chunk."""
    return max(STREAM_CHUNK, int(frame_batch_size) // STREAM_CHUNK * STREAM_CHUNK)


def _stream_batches(T, frame_batch_size):
    """[(t0, t1)] frame batches of the streamed passes: every boundary but the last is a multiple of 1024."""
    nb = _stream_batch_frames(frame_batch_size)
    return [(t0, min(T, t0 + nb)) for t0 in range(0, int(T), nb)]


def _gather_maps(frames, batches):
    """For each batch (t0, t1): (rows of the batch, rows of the destination) of the listed frames it carries.
    Destination row j holds frames[j], so a position of `frames` is covered exactly once (repeats included)."""
    fr = np.asarray(frames, dtype=np.int64).reshape(-1)
    maps = []
    for t0, t1 in batches:
        dst = np.nonzero((fr >= t0) & (fr < t1))[0]
        maps.append(((fr[dst] - t0).astype(np.int32), dst.astype(np.int32)))
    return maps


def _stream_source_problem(dataset_obj, distributed):
    """Why dataset_obj cannot be streamed (None: it can)."""
    if distributed:
        return "stream=True is single-GPU only (distributed=True is not supported)"
    if hasattr(dataset_obj, "slab"):
        return "stream=True does not support sources that build their frames on the device (.slab)"
    try:
        import torch
    except ImportError:     # pragma: no cover - torch is a dependency
        return None
    if isinstance(dataset_obj, torch.Tensor) and dataset_obj.device.type != "cpu":
        return "stream=True needs a host source (NumPy array / memmap, lazy_data_loader or CPU tensor), not a device tensor"
    return None


def _plan_mode(stream, T, D, free_bytes, streamable=True):
    """'resident' or 'stream'.  stream=None (auto) streams only when the resident plan cannot fit: it holds the raw
    fp32 movie and a standardised copy of it at the same time, twice the 4 D T bytes the single_copy rule estimates,
    so every movie that decomposes resident today stays resident."""
    if stream is None:
        return "stream" if streamable and 2.0 * 4.0 * D * T > free_bytes else "resident"
    return "stream" if stream else "resident"


def _usable_free_bytes(free, reserved, allocated):
    """Device memory a new allocation can get: what the driver reports free plus the blocks PyTorch's caching allocator
    holds reserved but unused (an earlier large call leaves them cached; the allocator reuses them, and releases them to
    retry before it reports out of memory)."""
    return int(free) + max(0, int(reserved) - int(allocated))


def _device_free_bytes(device):
    torch = _torch()
    return _usable_free_bytes(torch.cuda.mem_get_info(device)[0], torch.cuda.memory_reserved(device),
                              torch.cuda.memory_allocated(device))


def _stream_fit_bytes(esize, D, rows_alloc, ld_fit, n_fit, n_sample, nb, tile_bytes):
    """Device bytes the streamed mode needs around the fit frames: raw fit frames and sample (source dtype), the two
    batch buffers, the standardised / filtered fit frames (fp32, pixel-major) plus one more array of that size for the
    background-filter and pooling temporaries, and the tile stage (tile_bytes).  An estimate: small tables and the
    workspaces of single kernels are left out."""
    return esize * D * (n_fit + n_sample + 2 * nb) + 2 * 4 * rows_alloc * ld_fit + tile_bytes


def _stream_dtype(src):
    """Element type a source is staged and uploaded in: its own for uint16 / int16, fp32 otherwise."""
    dt = getattr(src, "dtype", None)
    try:
        dt = np.dtype(dt) if dt is not None else np.dtype(np.float32)
    except TypeError:
        dt = np.dtype(np.float32)
    return dt if dt in (np.dtype(np.uint16), np.dtype(np.int16)) else np.dtype(np.float32)


class _StreamedMovie:
    """The movie left at its source and read in frame batches: pass 1 (statistics, gathering the fit frames and the
    background sample), pass 2 (standardise + project every batch, in _ZBuilder).  Same staged upload as _Movie
    (_StagingRing); a batch is uploaded into one of two device buffers while the other one's kernels run."""

    def __init__(self, ctx, dataset_obj, frame_batch_size, num_workers=0):
        torch = _torch()
        self.ctx = ctx
        if isinstance(dataset_obj, torch.Tensor):
            dataset_obj = dataset_obj.detach().numpy()
        self.src = dataset_obj
        self.T, self.d1, self.d2 = (int(x) for x in dataset_obj.shape)
        self.D = self.d1 * self.d2
        self.rows_alloc = _round_up(self.D, 1024) + 1024
        self.np_dtype = _stream_dtype(dataset_obj)
        self.elem = _ELEM[self.np_dtype]
        self.tdtype = torch.from_numpy(np.zeros(1, dtype=self.np_dtype)).dtype
        self.batches = _stream_batches(self.T, frame_batch_size)
        self.nb = self.batches[0][1] - self.batches[0][0]
        self.project_frames = min(self.nb, STREAM_PROJECT_FRAMES)
        self.num_workers = num_workers
        self.bytes_uploaded = 0
        self.fit = self.sample = None     # gathered raw frames (device, frames-first)

    def check_fit_frames(self, n_fit, n_sample, tile_bytes):
        """Raise a ValueError (instead of a device out-of-memory error later) when the fit frames and the arrays of the
        tile stage built on them cannot fit next to the two batch buffers (_stream_fit_bytes)."""
        need = _stream_fit_bytes(self.np_dtype.itemsize, self.D, self.rows_alloc, int(self.ctx.lib.pmd_time_ld(n_fit)), n_fit,
                                 n_sample, self.nb, tile_bytes)
        free = _device_free_bytes(self.ctx.device)
        if need > free:
            raise ValueError("stream=True: fitting on {} frames of {} pixels needs about {:.1f} GB of device memory, {:.1f} GB "
                             "are free; lower frame_range (or frame_batch_size)".format(n_fit, self.D, need / 1e9, free / 1e9))

    def run_pass(self, consume):
        """Read the whole movie once; consume(batch, t0, n) enqueues the work on batch (device, (n, D), raw dtype)
        on the current stream.  Returns after the last batch is enqueued."""
        torch = _torch()
        ctx, D = self.ctx, self.D
        with _StagingRing(ctx, self.src, self.tdtype, self.nb, self.num_workers) as ring:
            main = ring.main
            dev = [torch.empty((self.nb, D), dtype=self.tdtype, device=ctx.device) for _ in range(min(2, len(self.batches)))]
            free = [None] * len(dev)             # event behind the kernels that last read a batch buffer
            for k, (b0, b1) in enumerate(self.batches):
                j = k % len(dev)
                if free[j] is not None:
                    ring.copy_stream.wait_event(free[j])
                main.wait_event(ring.upload(dev[j], b0, b1))     # the batch's last piece
                self.bytes_uploaded += (b1 - b0) * D * self.np_dtype.itemsize
                consume(dev[j][:b1 - b0], b0, b1 - b0)
                free[j] = torch.cuda.Event()
                free[j].record(main)

    streamed = True
    statistics_phase = "stream_stats"

    def statistics(self, compute_normalizer, mean, std, frames=None, sample=None):
        """Pass 1: chunk statistics of every batch, and the fit frames / background sample gathered in the source
        dtype.  Finishes mean / std."""
        torch = _torch()
        ctx, lib, T, D = self.ctx, self.ctx.lib, self.T, self.D
        ws = torch.empty(int(lib.pmd_stats_stream_workspace_bytes(T, D)), dtype=torch.uint8, device=ctx.device)
        self.fit = torch.empty((len(frames), D), dtype=self.tdtype, device=ctx.device)
        self.sample = torch.empty((len(sample), D), dtype=self.tdtype, device=ctx.device) if sample else None
        maps = [(m, _gather_maps(lst, self.batches), buf) for m, lst, buf in
                (("fit", frames, self.fit), ("sample", sample or [], self.sample)) if buf is not None]
        # the index maps of every batch go up in one table
        tables = []
        for _, per_batch, _ in maps:
            for src_rows, dst_rows in per_batch:
                tables += [src_rows, dst_rows]
        offs = np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int64)
        idx_dev = _i32(ctx, np.concatenate(tables) if tables else np.zeros(1, np.int32))
        k_batch = {t0: k for k, (t0, _) in enumerate(self.batches)}

        def consume(batch, t0, n):
            ctx.call("pmd_stats_stream_accumulate", ptr(batch), self.elem, t0, n, T, D, 1 if compute_normalizer else 0,
                     ptr(ws), ws.numel())
            k = k_batch[t0]
            for i, (_, per_batch, buf) in enumerate(maps):
                slot = 2 * (i * len(self.batches) + k)
                cnt = len(per_batch[k][0])
                if cnt:
                    ctx.call("pmd_gather_frames", ptr(batch), self.elem, D, ptr(idx_dev[int(offs[slot]):]),
                             ptr(idx_dev[int(offs[slot + 1]):]), cnt, ptr(buf))

        self.run_pass(consume)
        ctx.call("pmd_stats_stream_finish", T, D, 1 if compute_normalizer else 0, ptr(mean), ptr(std), ptr(ws), ws.numel())
        ctx.sync()     # the index table and the workspace are released on return

    def standardized(self, which, mean, std, frames=None):
        """Pixel-major (rows_alloc x ld) standardised copy of the "fit" or "sample" frames gathered in pass 1 (in list
        order; `frames` is not needed again).  "all": there is no whole-movie copy - None and the leading dimension of
        the blocks that pass 2 (project) hands out instead."""
        torch = _torch()
        ctx = self.ctx
        if which == "all":
            return None, int(ctx.lib.pmd_time_ld(self.project_frames))
        raw = self.fit if which == "fit" else self.sample
        nf = raw.shape[0]
        ld = ctx.lib.pmd_time_ld(nf)
        out = torch.empty((self.rows_alloc, ld), dtype=torch.float32, device=ctx.device)
        out[self.D:].zero_()
        ctx.call("pmd_standardize_transpose_typed", ptr(raw), self.elem, self.D, None, nf, ptr(mean), ptr(std), ptr(out), ld)
        return out, ld

    def release(self):
        """The standardised fit frames are written: the raw gathered frames are not read again."""
        self.fit = self.sample = None

    def project(self, mean, std, on_block):
        """Pass 2: every frame block of at most STREAM_PROJECT_FRAMES frames standardised into a pixel-major scratch
        (rows_alloc x pmd_time_ld(block)); on_block(xs, ld, t0, n) enqueues its projections."""
        torch = _torch()
        ctx, D = self.ctx, self.D
        nblk = self.project_frames
        ld = int(ctx.lib.pmd_time_ld(nblk))
        xs = torch.empty((self.rows_alloc, ld), dtype=torch.float32, device=ctx.device)
        xs[D:].zero_()
        esize = self.np_dtype.itemsize

        def consume(batch, t0, n):
            for s0 in range(0, n, nblk):
                sn = min(nblk, n - s0)
                ctx.call("pmd_standardize_transpose_typed", C.c_void_p(batch.data_ptr() + s0 * D * esize), self.elem, D,
                         None, sn, ptr(mean), ptr(std), ptr(xs), ld)
                on_block(xs, ld, t0 + s0, sn)

        self.run_pass(consume)
