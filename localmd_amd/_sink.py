"""
Where a movie-to-movie pass puts its frames, and the one scaffold that runs such a pass: the layer below export_movie,
dff_movie, register_movie / apply_shifts and register_piecewise / apply_field, beside _stream.

A destination (_Dest, made by _destination from what the caller passed as ``out``) is a .tif / .tiff or .npy path, a host
array or a contiguous device tensor.  A sink gives every 1024-frame block a device address to be written to: _DeviceSink
the block's place in the device tensor, _HostSink one of HOST_SLOTS device buffers whose copy to a page-locked buffer
runs on a side stream while a writer thread puts the frames into the file or array and the next block computes.

``movie_pass`` is the scaffold.  It opens the destination, builds the sink, hands every block of the caller's pass to
the caller's ``write`` with the address it goes to, and orders the ends: finish, sync, shutdown, close on success; on any
failure (a writer-thread error and a KeyboardInterrupt included) sink.abort, dest.abort, which removes a file this call
created, and shutdown, and the error goes on to the caller.  The front-door checks the callers share (check_bigtiff,
device_index, _optional_destination) are here too.  No helper knows its caller.
"""
import ctypes
import itertools
import os
import queue
import threading

import numpy as np

HOST_SLOTS = 2          # device + page-locked output buffers of a host destination
COPY_THREADS = 8        # threads that copy a block into a NumPy destination


# ---- front-door checks (no device work, no file) --------------------------------------------------------------------
def check_bigtiff(bigtiff):
    if bigtiff is not None and not isinstance(bigtiff, bool):
        raise ValueError("bigtiff must be None, True or False")


def device_index(pmd, device, ctx):
    """The device the pass runs on: that of ``pmd.to_device()`` when it is active, else the caller's ``ctx``'s, else
    ``device`` (0 when None)."""
    dv = getattr(pmd, "_dev", None)
    if dv is not None:
        return dv["ctx"].device_index
    return ctx.device_index if ctx is not None else (0 if device is None else int(device))


# ---- destinations ---------------------------------------------------------------------------------------------------
def _torch_dtype(np_dtype):
    import torch

    return {np.dtype(np.float32): torch.float32, np.dtype(np.int16): torch.int16,
            np.dtype(np.uint16): getattr(torch, "uint16", None)}[np.dtype(np_dtype)]


class _Dest:
    """Where the frames go: kind in {"tiff", "npy", "device", "array"}."""

    def __init__(self, kind, target, shape, dtype, bigtiff=None):
        self.kind, self.target, self.shape, self.dtype, self.bigtiff = kind, target, shape, dtype, bigtiff
        self.writer = None      # TiffWriter / open_memmap once opened
        self.pool = None        # copy threads of a NumPy destination

    def open(self):
        from ._minitiff import TiffWriter

        if self.kind == "tiff":
            self.writer = TiffWriter(self.target, self.shape, self.dtype, bigtiff=self.bigtiff)
        elif self.kind == "npy":
            self.writer = np.lib.format.open_memmap(self.target, mode="w+", dtype=self.dtype, shape=self.shape)

    def put(self, t0, block):
        """Frames t0 .. t0 + len(block) (a NumPy array), in frame order."""
        if self.kind == "tiff":
            self.writer.write(block)
        elif self.kind == "npy" or isinstance(self.target, np.ndarray):
            tgt = self.writer if self.kind == "npy" else self.target
            self._copy(tgt[t0:t0 + len(block)], block)
        else:
            tgt = self.target
            try:
                import torch

                if isinstance(tgt, torch.Tensor):
                    tgt[t0:t0 + len(block)] = torch.from_numpy(block)
                    return
            except ImportError:     # pragma: no cover - torch is a dependency
                pass
            tgt[t0:t0 + len(block)] = block

    def _copy(self, dst, src):
        """dst[...] = src in frame ranges on COPY_THREADS threads (NumPy copies release the GIL; one thread moves well
        under the device-to-host rate)."""
        n = len(src)
        parts = max(1, min(COPY_THREADS, n))
        if parts == 1:
            dst[...] = src
            return
        if self.pool is None:
            from concurrent.futures import ThreadPoolExecutor

            self.pool = ThreadPoolExecutor(max_workers=COPY_THREADS)
        edges = [n * k // parts for k in range(parts + 1)]
        for f in [self.pool.submit(dst[a:b].__setitem__, Ellipsis, src[a:b]) for a, b in zip(edges, edges[1:])]:
            f.result()

    def shutdown(self):
        if self.pool is not None:
            self.pool.shutdown()
            self.pool = None

    def close(self):
        if self.kind == "tiff":
            self.writer.close()
        elif self.kind == "npy":
            self.writer.flush()
            self.writer = None
        return self.target

    def abort(self):
        """Remove a file this export created (nothing to undo for a caller's array)."""
        if self.kind == "tiff" and self.writer is not None:
            self.writer.abort()
        elif self.kind == "npy":
            self.writer = None
            try:
                os.remove(self.target)
            except FileNotFoundError:
                pass


def _destination(out, shape, dtype, bigtiff, device_index):
    from ._minitiff import tiff_needs_bigtiff

    if isinstance(out, (str, os.PathLike)):
        path = os.fspath(out)
        ext = os.path.splitext(path)[1].lower()
        if ext in (".tif", ".tiff"):
            if bigtiff is False and tiff_needs_bigtiff(shape[0], shape[1], shape[2], dtype.itemsize):
                raise ValueError("{} frames of {} x {} {} do not fit in a classic TIFF (4 GiB); use bigtiff=True or "
                                 "bigtiff=None".format(shape[0], shape[1], shape[2], dtype))
            return _Dest("tiff", path, shape, dtype, bigtiff)
        if ext == ".npy":
            return _Dest("npy", path, shape, dtype)
        raise ValueError("out {!r}: unknown suffix {!r}; use .tif, .tiff or .npy, or pass an array".format(path, ext))
    if bigtiff is not None:
        raise ValueError("bigtiff applies to a .tif / .tiff destination only")
    try:
        got_shape = tuple(int(x) for x in out.shape)
    except (AttributeError, TypeError):
        raise TypeError("out must be a path or an array-like with a shape and a dtype, got {}".format(
            type(out).__name__)) from None
    if got_shape != tuple(shape):
        raise ValueError("out has shape {}, the export needs {}".format(got_shape, tuple(shape)))
    import torch

    if isinstance(out, torch.Tensor):
        if out.dtype != _torch_dtype(dtype):
            raise ValueError("out has dtype {}, the export writes {}".format(out.dtype, dtype))
        if out.device.type != "cpu":
            if not out.is_contiguous() or out.device != torch.device("cuda", device_index):
                raise ValueError("a device tensor destination must be contiguous and on cuda:{} (got {}{})".format(
                    device_index, out.device, "" if out.is_contiguous() else ", not contiguous"))
            return _Dest("device", out, shape, dtype)
        return _Dest("array", out, shape, dtype)
    try:
        got = np.dtype(out.dtype)
    except (AttributeError, TypeError):
        raise TypeError("out has no NumPy dtype ({})".format(type(out).__name__)) from None
    if got != dtype:
        raise ValueError("out has dtype {}, the export writes {}".format(got, dtype))
    return _Dest("array", out, shape, dtype)


def _optional_destination(out, shape, dtype, bigtiff, device_index):
    """_destination, or None for ``out=None`` (a pass that only estimates)."""
    if out is None:
        if bigtiff is not None:
            raise ValueError("bigtiff applies to a .tif / .tiff destination only")
        return None
    return _destination(out, shape, dtype, bigtiff, device_index)


# ---- sinks ----------------------------------------------------------------------------------------------------------
class _HostSink:
    """Output blocks to the host: HOST_SLOTS device buffers and as many page-locked ones; block k uses slot k mod
    HOST_SLOTS.  Its copy to the host runs on a side stream, and a writer thread puts it into the destination while the
    next blocks compute.  An error in the writer thread is raised in the caller."""

    def __init__(self, ctx, dest, frame_bytes, frame_shape, np_dtype, block):
        import torch

        self.torch = torch
        self.ctx, self.dest = ctx, dest
        self.frame_bytes, self.frame_shape, self.np_dtype = frame_bytes, frame_shape, np_dtype
        nbytes = block * frame_bytes
        self.dev = [torch.empty(nbytes, dtype=torch.uint8, device=ctx.device) for _ in range(HOST_SLOTS)]
        self.pin = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(HOST_SLOTS)]
        self.copied = [None] * HOST_SLOTS                   # event behind the last device-to-host copy out of a slot
        self.consumed = [threading.Event() for _ in range(HOST_SLOTS)]
        for e in self.consumed:
            e.set()
        self.side = torch.cuda.Stream(device=ctx.device)
        self.q = queue.Queue()
        self.error = None
        self.thread = threading.Thread(target=self._writer, daemon=True)
        self.thread.start()

    def _writer(self):
        while True:
            item = self.q.get()
            if item is None:
                return
            fin, j, t0, m = item
            try:
                if self.error is None:
                    fin.synchronize()
                    block = self.pin[j][:m * self.frame_bytes].numpy().view(self.np_dtype).reshape((m,) + self.frame_shape)
                    self.dest.put(t0, block)
            except BaseException as e:      # noqa: BLE001 - handed to the caller
                self.error = e
            finally:
                self.consumed[j].set()

    def dst(self, k, t0):
        """Device pointer the kernel writes block k (frames from t0) to."""
        j = k % HOST_SLOTS
        if self.copied[j] is not None:
            self.torch.cuda.current_stream(self.ctx.device).wait_event(self.copied[j])
        return self.dev[j].data_ptr()

    def done(self, k, t0, m):
        torch = self.torch
        j = k % HOST_SLOTS
        self.consumed[j].wait()         # the writer has put the slot's previous block
        self._raise()
        self.consumed[j].clear()
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.ctx.device))
        self.side.wait_event(ev)
        with torch.cuda.stream(self.side):
            self.pin[j][:m * self.frame_bytes].copy_(self.dev[j][:m * self.frame_bytes], non_blocking=True)
            fin = torch.cuda.Event()
            fin.record(self.side)
        self.copied[j] = fin
        self.q.put((fin, j, t0, m))

    def _raise(self):
        if self.error is not None:
            raise self.error

    def finish(self):
        self.q.put(None)
        self.thread.join()
        self._raise()

    def abort(self):
        self.error = self.error or RuntimeError("export aborted")
        self.q.put(None)
        self.thread.join()
        self.side.synchronize()


class _DeviceSink:
    """Output blocks straight into a contiguous device tensor."""

    def __init__(self, out, frame_bytes):
        self.base, self.frame_bytes = out.data_ptr(), frame_bytes

    def dst(self, k, t0):
        return self.base + t0 * self.frame_bytes

    def done(self, k, t0, m):
        pass

    def finish(self):
        pass

    def abort(self):
        pass


class _NoSink:
    """The sink of a pass without a destination: no address, nothing to finish."""

    def dst(self, k, t0):
        return None

    def done(self, k, t0, m):
        pass

    def finish(self):
        pass

    def abort(self):
        pass


def _make_sink(ctx, dest, frame_shape, np_dtype, capacity):
    """The sink of ``dest`` for frames of ``frame_shape`` and ``np_dtype`` in blocks of at most ``capacity`` frames."""
    frame_bytes = int(np.prod(frame_shape)) * np.dtype(np_dtype).itemsize
    if dest.kind == "device":
        return _DeviceSink(dest.target, frame_bytes)
    return _HostSink(ctx, dest, frame_bytes, tuple(frame_shape), np_dtype, capacity)


# ---- the scaffold ---------------------------------------------------------------------------------------------------
def movie_pass(ctx, dest, frame_shape, np_dtype, capacity, blocks, write):
    """One pass that writes a movie of ``frame_shape`` frames of ``np_dtype`` into ``dest`` (a _Dest, or None: a pass
    that only looks).  ``blocks(each)`` is the caller's walk: it calls ``each(c0, m, yp, elem)`` for every block (m
    frames from c0 on, at most ``capacity``, in frame order; _stream.each_block is the usual one) and returns when the
    last one is enqueued.  ``write(c0, m, yp, elem, out)`` enqueues the kernels that write the block's frames to the
    device address ``out`` (a ctypes.c_void_p; None without a destination).  Returns ``dest.close()``, the path or the
    array (None without a destination).

    Success: open, sink, blocks, sink.finish, ctx.sync, dest.shutdown, dest.close.  Any BaseException, from a block, from
    the writer thread (it surfaces in sink.done or sink.finish) or from the sync: sink.abort, dest.abort, dest.shutdown,
    and the same exception goes on; close is not called."""
    if dest is None:
        dest = _Dest(None, None, None, None)           # nothing to open, put, remove or return
    sink, count = _NoSink(), itertools.count()
    dest.open()
    try:
        if dest.kind is not None:
            sink = _make_sink(ctx, dest, frame_shape, np_dtype, capacity)

        def each(c0, m, yp, elem):
            k = next(count)
            at = sink.dst(k, c0)
            write(c0, m, yp, elem, None if at is None else ctypes.c_void_p(at))
            sink.done(k, c0, m)

        blocks(each)
        sink.finish()
        ctx.sync()
    except BaseException:
        sink.abort()
        dest.abort()
        raise
    finally:
        dest.shutdown()
    return dest.close()
