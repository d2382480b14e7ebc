"""
One pass over a movie against a stored decomposition: what project_frames / project_movie, make_pmd_diagnostic_images,
export_movie, extract_traces, regressor_maps, summary_images, quantile_images and the rolling baseline (baseline.py)
share.  The device context of a PMDArray, how a source is read (host sources through the pinned staging ring of the
streamed decomposition, device tensors sliced in place), the 1024-frame reconstruction blocks, the walk over the
blocks of a batch and the Vt columns of one, the uploaded statistics and R s, the host ring that results leave the
device through, and the argument and device-memory checks the callers have in common (check_pmd, name_tuple,
check_fit, _check_count, _is_int).  Rebuilding a block of the denoised or residual movie from these is _expand's, and
so are the plan and the one block walk of the five consumers that keep per-pixel state (KindPlan, KindBlocks); where a
pass that writes a movie puts its frames (destinations, sinks, and the scaffold that opens, finishes and aborts them,
movie_pass) is _sink's, the module beside this one.  The movie sources, the frame-batch plan and the element types are
_movie.py's, the layer below this one and below the decomposition driver.  No helper knows its caller.
"""
import contextlib

import numpy as np

from ._movie import _StreamedMovie, _device_elem, _stream_batches, _stream_dtype

BLOCK = 1024            # frames per reconstruction block; blocks start on multiples of it


# ---- argument checks and plans (no device work) ---------------------------------------------------------------------
def check_pmd(pmd):
    from .pmdarray import PMDArray

    if not isinstance(pmd, PMDArray):
        raise TypeError("pmd must be a localmd_amd.PMDArray, got {}".format(type(pmd).__name__))


def name_tuple(value, allowed, word, words):
    """``value``, one name or an iterable of distinct names from ``allowed``, as a tuple; ``word`` / ``words`` say what
    a name is in the error messages ("panel" / "panels")."""
    if isinstance(value, str):
        value = (value,)
    try:
        value = tuple(value)
    except TypeError:
        raise ValueError("{} must be a name or a tuple of names from {}".format(words, allowed)) from None
    if not value:
        raise ValueError("{} is empty; choose from {}".format(words, allowed))
    for v in value:
        if not isinstance(v, str) or v not in allowed:
            raise ValueError("unknown {} {!r}; choose from {}".format(word, v, allowed))
    if len(set(value)) != len(value):
        raise ValueError("{} {} name a {} twice".format(words, value, word))
    return value


def check_fit(what, need, free, hint="; lower frame_batch_size"):
    """ValueError when ``what`` needs more device bytes than are free; ``hint`` is the advice the message ends in, with
    the punctuation that joins it on."""
    if need > free:
        raise ValueError("{} needs about {:.2f} GB of device memory, {:.2f} GB are free{}".format(
            what, need / 1e9, free / 1e9, hint))


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _check_count(value, name):
    if not _is_int(value) or int(value) < 1:
        raise ValueError("{} must be an integer >= 1, got {!r}".format(name, value))
    return int(value)


def batch_buffer_bytes(nb, D, esize, host_source, n_batches):
    """Device bytes of the frame batches: two buffers for a host source of more than one batch, else one (a converted
    copy at most for a device tensor)."""
    return (2 if host_source and n_batches > 1 else 1) * nb * D * esize


def block_plan(T, frame_batch_size, block=BLOCK):
    """[(b0, b1, [(c0, c1), ...])]: the frame batches the movie is read in (those of the streamed decomposition, whole
    1024-frame chunks) and the reconstruction blocks of each: ``block`` frames from the batch's start on, the last one
    shorter.  With block = BLOCK the blocks start on multiples of it and are the same for every frame_batch_size."""
    return [(b0, b1, [(c0, min(b1, c0 + block)) for c0 in range(b0, b1, block)])
            for b0, b1 in _stream_batches(T, frame_batch_size)]


def factor_bytes(n_cols, rank, factors_on_device):
    """Device bytes of the factors a block product reads: one block of Vt columns (VtBlocks), and R s (scaled_r) unless
    the PMDArray already holds it on the device; nothing for a decomposition without columns or rank."""
    if rank <= 0 or n_cols <= 0:
        return 0
    return 4 * rank * BLOCK + (0 if factors_on_device else 4 * n_cols * rank)


def block_walk(plan, D):
    """walk(batch, b0) for the ``consume`` of read_batches: yields (c0, m, yp) for every reconstruction block of the
    batch of ``plan`` (block_plan) that starts at frame b0: its m frames from c0 on and the device address of frame c0
    in the batch of D-pixel frames, None without a movie."""
    import ctypes as C

    blocks_of = {b0: blocks for b0, _, blocks in plan}

    def walk(batch, b0):
        for c0, c1 in blocks_of[b0]:
            yield c0, c1 - c0, (C.c_void_p(batch.data_ptr() + (c0 - b0) * D * batch.element_size())
                                if batch is not None else None)

    return walk


def source_info(movie, shape):
    """(on_device, element size the movie is uploaded / read in) of a movie that must have ``shape``."""
    import torch

    got = tuple(int(x) for x in movie.shape)
    if got != tuple(shape):
        raise ValueError("the movie has shape {}, the decomposition {}".format(got, tuple(shape)))
    if isinstance(movie, torch.Tensor) and movie.device.type != "cpu":
        return True, movie.element_size() if _device_elem(movie[:0]) is not None else 4
    src = movie.detach().numpy() if isinstance(movie, torch.Tensor) else movie
    return False, _stream_dtype(src).itemsize


# ---- device side ----------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def device_context(pmd, device, ctx):
    """(ctx, dv): the context and uploaded factors of ``pmd.to_device()`` when it is active (dv is None otherwise), else
    the caller's ``ctx``, else a new Context on ``device`` (0 when None) that is closed on exit."""
    from . import _lib

    dv = getattr(pmd, "_dev", None)
    own = False
    if dv is not None:
        ctx = dv["ctx"]
    elif ctx is None:
        ctx = _lib.Context(0 if device is None else int(device))
        own = True
    try:
        yield ctx, dv
    finally:
        if own:
            ctx.close()


def upload_f32(ctx, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(ctx.device)


def mean_std(ctx, pmd):
    """The mean and std images as fp32 device vectors in C pixel order (the pixel ids of the group and ROI tables are
    C-order whatever pmd.order is; pmd.var_img is the std image, stored under the reference's name)."""
    return upload_f32(ctx, np.asarray(pmd.mean_img).reshape(-1)), upload_f32(ctx, np.asarray(pmd.var_img).reshape(-1))


def scaled_r(ctx, pmd, dv):
    """R diag(s) (n_cols x rank, fp32) on the device: the copy of pmd.to_device() or an upload."""
    return dv["rs"] if dv is not None else upload_f32(ctx, pmd.r * pmd.s[None, :])


def read_batches(ctx, movie, batches, frame_batch_size, num_workers, consume):
    """Read ``movie`` once: consume(batch, elem, b0, n) enqueues the work on a contiguous (n, D) device batch of element
    type elem that starts at frame b0.  A device tensor is sliced in place along ``batches`` = [(b0, b1), ...] (element
    types the kernels do not read are converted to fp32); any other source goes through the pinned staging ring of the
    streamed decomposition in its own batches of frame_batch_size; without a movie every batch is None."""
    import torch

    if movie is None:
        for b0, b1 in batches:
            consume(None, 0, b0, b1 - b0)
    elif isinstance(movie, torch.Tensor) and movie.device.type != "cpu":
        for b0, b1 in batches:
            b = movie[b0:b1].to(ctx.device).reshape(b1 - b0, -1)
            elem = _device_elem(b)
            if elem is None:
                b, elem = b.to(torch.float32), 0
            consume(b.contiguous(), elem, b0, b1 - b0)
    else:
        src = _StreamedMovie(ctx, movie, frame_batch_size, num_workers=num_workers)
        src.run_pass(lambda batch, b0, n: consume(batch, src.elem, b0, n))


def each_block(ctx, movie, plan, D, frame_batch_size, num_workers):
    """blocks(each) for _sink.movie_pass: reads ``movie`` once along ``plan`` (read_batches; None: no movie is read) and
    calls each(c0, m, yp, elem) for every reconstruction block (block_walk), in frame order."""
    walk = block_walk(plan, D)

    def blocks(each):
        def consume(batch, elem, b0, n):
            for c0, m, yp in walk(batch, b0):
                each(c0, m, yp, elem)

        read_batches(ctx, movie, [(b0, b1) for b0, b1, _ in plan], frame_batch_size, num_workers, consume)

    return blocks


class VtBlocks:
    """The columns of Vt of one reconstruction block in ``buf`` (rank x BLOCK on the device, the same leading dimension
    for every block and source): copied from the Vt of pmd.to_device(), else uploaded through two page-locked buffers."""

    def __init__(self, ctx, pmd, dv):
        import torch

        self.torch, self.dev, self.pmd, self.dv = torch, ctx.device, pmd, dv
        self.buf = torch.empty((int(pmd.r.shape[1]), BLOCK), dtype=torch.float32, device=ctx.device)
        self.pin, self.ev, self.k = [None, None], [None, None], 0

    def load(self, c0, m):
        """buf[:, :m] = Vt[:, c0:c0 + m], enqueued on the current stream."""
        torch, buf = self.torch, self.buf
        if self.dv is not None:
            buf[:, :m].copy_(self.dv["v"][:, c0:c0 + m])
            return
        j = self.k % 2
        self.k += 1
        if self.pin[j] is None:
            self.pin[j] = torch.empty(buf.shape, dtype=torch.float32, pin_memory=True)
        elif self.ev[j] is not None:
            self.ev[j].synchronize()            # the upload that last read this buffer has finished
        np.copyto(self.pin[j][:, :m].numpy(), self.pmd.v[:, c0:c0 + m], casting="unsafe")
        buf[:, :m].copy_(self.pin[j][:, :m], non_blocking=True)
        self.ev[j] = torch.cuda.Event()
        self.ev[j].record(torch.cuda.current_stream(self.dev))


class ToHost:
    """(rows x n) fp32 results batch by batch to host memory: two device buffers and two page-locked buffers, the copy
    of a batch overlaps the next batch's work; the result has no length bound on the device."""

    def __init__(self, ctx, rows, n):
        import torch

        self.ctx, self.rows = ctx, rows
        self.out = np.empty((rows, n), dtype=np.float32)
        self.dev, self.host, self.pending = [None, None], [None, None], []
        self.k = 0
        self.torch = torch
        self.stream = torch.cuda.Stream(device=ctx.device)   # not the upload stream of the staging ring

    def dst(self, t0, nb):
        """(device buffer, leading dimension) of the rows x nb results of the batch that starts at t0."""
        torch = self.torch
        j = self.k % 2
        if self.dev[j] is None or self.dev[j].numel() < self.rows * nb:
            self.dev[j] = torch.empty(self.rows * nb, dtype=torch.float32, device=self.ctx.device)
            self.host[j] = torch.empty(self.rows * nb, dtype=torch.float32, pin_memory=True)
        return self.dev[j], nb

    def done(self, t0, nb):
        torch = self.torch
        j = self.k % 2
        self.k += 1
        main = torch.cuda.current_stream(self.ctx.device)
        side = self.stream
        ev = torch.cuda.Event()
        ev.record(main)
        side.wait_event(ev)
        with torch.cuda.stream(side):
            self.host[j][:self.rows * nb].copy_(self.dev[j][:self.rows * nb], non_blocking=True)
            fin = torch.cuda.Event()
            fin.record(side)
        # a buffer pair is written again two batches later: finish the older copy first
        self.pending.append((fin, j, t0, nb))
        if len(self.pending) == 2:
            self._drain(self.pending.pop(0))

    def _drain(self, item):
        fin, j, t0, nb = item
        fin.synchronize()
        self.out[:, t0:t0 + nb] = self.host[j][:self.rows * nb].numpy().reshape(self.rows, nb)

    def finish(self):
        while self.pending:
            self._drain(self.pending.pop(0))
