"""
Streamed export of a decomposition: the denoised movie, the residual and the raw movie, side by side, to a TIFF, an
.npy file, a host array or a device tensor.

``export_movie(pmd, out, movie, panels=("raw", "denoised", "residual"))`` writes the raw | denoised | residual
"triptych" that the reference's demo builds with ``np.concatenate([movie, pmd[:], movie - pmd[:]], axis=2)`` and
``tifffile.imwrite`` (demos/official_demo.ipynb, last cell), without ever holding the movie, or any copy of it, in
memory.  Values, all fp32: ``y`` the source value, ``x = mean_img + var_img * (U R diag(s) Vt)`` (what ``pmd[t]``
approximates), ``r = y - x`` from the rounded ``x``; integer outputs round half to even and saturate (quantize).

Hot path: the movie is read once in the frame batches of the streamed decomposition; each 1024-frame reconstruction
block (blocks start on multiples of 1024 whatever the batch size, so every product has the same shape and every output
bit is the same for every batching and source) goes through ``pmd_gemm`` (C = (R s) Vt[:, block]) and one fused kernel,
``pmd_group_expand`` (csrc/expand_fused.hip), from C to finished output frames.  The kernel walks, per 64-pixel patch,
the groups of U's columns that touch it (projection.group_tables, cached on the PMDArray and shared with project_frames;
the per-patch lists are built here).  Reading the movie and the block plan are those of _stream, the two calls of a
block those of _expand.Expander, shared with regressor_maps, summary_images and quantile_images.  Host destinations get
each block through a ring of two device and two page-locked buffers: the copy to the host runs on a side stream and a
writer thread puts the frames into the file or array while the next block computes.  Device memory and host memory do
not grow with the movie's length.
"""
import itertools
import os
import queue
import threading

import numpy as np

from ._expand import ENTRY_FIELDS, EXPORT_PATCH, _PANEL_CODE, Expander, expander_bytes, panel_code  # noqa: F401
from ._movie import _ELEM, _device_free_bytes
from ._stream import BLOCK as EXPORT_BLOCK, block_plan as export_plan
from ._stream import (batch_buffer_bytes, block_walk, check_fit, device_context, name_tuple, read_batches,
                      source_info)
from .projection import MAX_ROWS, P_MAX, ROW_PAD, _pad, tables_for

HOST_SLOTS = 2          # device + page-locked output buffers of a host destination
COPY_THREADS = 8        # threads that copy a block into a NumPy destination
PANELS = ("raw", "denoised", "residual")
_OUT_DTYPES = {"float32": np.float32, "uint16": np.uint16, "int16": np.int16}


def quantize(v, dtype):
    """The conversion of pmd_group_expand in NumPy: float32 as is; uint16 / int16 round half to even, saturate to the
    type's range, NaN -> 0."""
    dtype = np.dtype(dtype)
    v = np.asarray(v, dtype=np.float32)
    if dtype == np.float32:
        return v.copy()
    info = np.iinfo(dtype)
    with np.errstate(invalid="ignore"):
        q = np.clip(np.rint(v), info.min, info.max)
    return np.where(np.isnan(q), 0, q).astype(dtype)


# ---- per-patch tables ----------------------------------------------------------------------------------------------
def expand_tables(tabs):
    """The per-patch entry lists of pmd_group_expand from the group tables of projection.group_tables.  Patch k holds
    the C-order pixels [64 k, 64 k + 64); it gets one entry per group with a pixel in it, in group order:

    patch_ptr int64 (n_patches + 1,)   entries of patch k: patch_ptr[k] .. patch_ptr[k + 1]
    entries   int64 (E, 4)             {a_off, p64, r, c_row0}: the group's block A_g, its row length, rows, first C row
    qmap      int32 (E * 64,)          index of the patch's pixel within the group's pixel list, -1 when not in it
    """
    g, pix, col0, D = tabs["groups"], tabs["pix"], tabs["col0"], int(tabs["D"])
    n_patches = -(-D // EXPORT_PATCH)
    G = len(g)
    if G == 0 or pix.size == 0:
        return {"patch_ptr": np.zeros(n_patches + 1, np.int64), "entries": np.zeros((0, ENTRY_FIELDS), np.int64),
                "qmap": np.zeros(0, np.int32), "n_patches": n_patches}
    p = g[:, 1]
    gid = np.repeat(np.arange(G, dtype=np.int64), p)
    q = np.arange(pix.size, dtype=np.int64) - np.repeat(g[:, 0], p)
    c = pix.astype(np.int64)
    key = (c // EXPORT_PATCH) * G + gid
    ukey, inv = np.unique(key, return_inverse=True)
    ent_patch, ent_g = ukey // G, ukey % G
    entries = np.stack([g[ent_g, 2], _pad(p[ent_g], 64), g[ent_g, 4], col0[ent_g]], axis=1).astype(np.int64)
    qmap = np.full(len(ukey) * EXPORT_PATCH, -1, dtype=np.int32)
    qmap[inv.reshape(-1) * EXPORT_PATCH + c % EXPORT_PATCH] = q
    patch_ptr = np.searchsorted(ent_patch, np.arange(n_patches + 1), side="left").astype(np.int64)
    return {"patch_ptr": patch_ptr, "entries": entries, "qmap": qmap, "n_patches": n_patches}


def validate_expand_tables(x, n_a, n_cols, D):
    """Raise ValueError unless every index pmd_group_expand follows stays inside its array (the kernel trusts them)."""
    pp, e, qm = x["patch_ptr"], x["entries"], x["qmap"]
    n_patches = -(-int(D) // EXPORT_PATCH)
    if pp.shape != (n_patches + 1,) or e.ndim != 2 or e.shape[1] != ENTRY_FIELDS or qm.shape != (len(e) * EXPORT_PATCH,):
        raise ValueError("expand tables: bad table shapes")
    if pp[0] != 0 or pp[-1] != len(e) or np.any(np.diff(pp) < 0):
        raise ValueError("expand tables: patch offsets are not monotone / do not cover the entries")
    if not len(e):
        return
    a_off, p64, r, c_row0 = (e[:, k] for k in range(ENTRY_FIELDS))
    if np.any(r < 1) or np.any(r > MAX_ROWS) or np.any(p64 < 64) or np.any(p64 % 64) or np.any(p64 > _pad(P_MAX, 64)):
        raise ValueError("expand tables: an entry has a row count outside [1, {}] or a bad row length".format(MAX_ROWS))
    if np.any(a_off < 0) or np.any(a_off + _pad(r, ROW_PAD) * p64 > n_a):
        raise ValueError("expand tables: an entry's block lies outside the value array")
    if np.any(c_row0 < 0) or np.any(c_row0 + r > n_cols):
        raise ValueError("expand tables: an entry's rows lie outside C")
    qq = qm.reshape(len(e), EXPORT_PATCH)
    if np.any(qq < -1) or np.any(qq >= p64[:, None]):
        raise ValueError("expand tables: a pixel index lies outside its group")


def expand_tables_for(pmd):
    """Group tables (cached on pmd._groups, shared with project_frames) and their per-patch lists (cached with them)."""
    tabs = tables_for(pmd)
    x = tabs.get("expand")
    if x is None:
        x = expand_tables(tabs)
        validate_expand_tables(x, int(tabs["a"].size), int(tabs["n_cols"]), int(tabs["D"]))
        tabs["expand"] = x
    return tabs, x


# ---- argument checks (no device work, no file) ---------------------------------------------------------------------
def _out_dtype(dtype):
    try:
        key = np.dtype(dtype).name
    except TypeError:
        key = None
    if key not in _OUT_DTYPES:
        raise ValueError("dtype must be one of {}, got {!r}".format(tuple(_OUT_DTYPES), dtype))
    return np.dtype(_OUT_DTYPES[key])


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


def export_device_bytes(D, nb, esize, n_panels, out_esize, n_cols, rank, n_entries, n_a, n_patches, needs_movie,
                        host_source, n_batches, host_dest, factors_on_device):
    """Device bytes export_movie holds for a movie of D pixels read in batches of nb frames; no term grows with the
    movie's length.  Batch buffers (two for a host source, a converted copy at most for a device tensor), one block of
    Vt columns and of C, the output ring of a host destination, the tables, mean and std, and R s unless the PMDArray
    already holds it on the device (expander_bytes; C is counted only where a product fills it)."""
    need = expander_bytes(D=D, n_cols=n_cols, rank=rank, n_entries=n_entries, n_a=n_a, n_patches=n_patches,
                          factors_on_device=factors_on_device, own_ct=rank > 0)
    if needs_movie:
        need += batch_buffer_bytes(nb, D, esize, host_source, n_batches)
    if host_dest:
        need += HOST_SLOTS * EXPORT_BLOCK * D * n_panels * out_esize
    return need + (1 << 20)     # the allocator's rounding of the small arrays


# ---- public entry point --------------------------------------------------------------------------------------------
def export_movie(pmd, out, movie=None, *, panels="denoised", dtype="float32", frame_batch_size=10000, num_workers=0,
                 bigtiff=None, device=None, ctx=None):
    """Write the frames of ``panels`` ("raw", "denoised", "residual", side by side along the width: output shape
    (T, d1, len(panels) d2)) to ``out``: a .tif / .tiff path (streamed multipage TIFF, BigTIFF when needed or when
    ``bigtiff=True``), an .npy path, or an existing array-like of the output shape and ``dtype`` (NumPy arrays and
    memmaps, CPU tensors, anything that takes ``out[t0:t1] = block`` in frame order; a contiguous device tensor on the
    context's device is written in place by the kernel).  Returns the path or the array.

    ``movie`` (needed by "raw" and "residual"): NumPy arrays and memmaps, any lazy_data_loader (TiffArray included),
    CPU tensors (read once in ``frame_batch_size`` batches through the pinned staging ring of the streamed
    decomposition, uint16 / int16 in their own dtype) and device tensors (sliced in place).  ``dtype``: "float32",
    "uint16" or "int16" (round half to even, saturating, NaN -> 0: quantize).  After ``pmd.to_device()`` its context
    and uploaded factors are reused.  Argument errors are raised before any device work and before a file is created;
    a file this call created is removed when it fails midway."""
    from .pmdarray import PMDArray

    if not isinstance(pmd, PMDArray):
        raise TypeError("pmd must be a localmd_amd.PMDArray, got {}".format(type(pmd).__name__))
    panels = name_tuple(panels, PANELS, "panel", "panels")
    out_dtype = _out_dtype(dtype)
    if bigtiff is not None and not isinstance(bigtiff, bool):
        raise ValueError("bigtiff must be None, True or False")
    T, d1, d2 = (int(x) for x in pmd.shape)
    D = d1 * d2
    needs_movie = any(p != "denoised" for p in panels)
    if needs_movie and movie is None:
        raise ValueError("panels {} need the movie: pass movie=".format(tuple(p for p in panels if p != "denoised")))
    on_device, esize = source_info(movie, pmd.shape) if movie is not None else (False, 4)
    dv = getattr(pmd, "_dev", None)
    dev_index = dv["ctx"].device_index if dv is not None else (ctx.device_index if ctx is not None else
                                                               (0 if device is None else int(device)))
    dest = _destination(out, (T, d1, len(panels) * d2), out_dtype, bigtiff, dev_index)
    plan = export_plan(T, frame_batch_size)
    nb = plan[0][1] - plan[0][0] if plan else 0
    tabs, xt = expand_tables_for(pmd)
    n_cols, rank = (int(x) for x in pmd.r.shape)

    with device_context(pmd, dev_index, ctx) as (ctx, dv):
        need = export_device_bytes(D, nb, esize, len(panels), out_dtype.itemsize, n_cols, rank, len(xt["entries"]),
                                   int(tabs["a"].size), int(xt["n_patches"]), needs_movie, not on_device, len(plan),
                                   dest.kind != "device", dv is not None)
        check_fit("export_movie", need, _device_free_bytes(ctx.device))
        dest.open()
        try:
            _export(ctx, pmd, dv, tabs, xt, movie if needs_movie else None, plan, panels, out_dtype, dest,
                    frame_batch_size, num_workers)
        except BaseException:
            dest.abort()
            raise
        finally:
            dest.shutdown()
        return dest.close()


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


def _export(ctx, pmd, dv, tabs, xt, movie, plan, panels, out_dtype, dest, frame_batch_size, num_workers):
    import ctypes as C

    T, d1, d2 = (int(x) for x in pmd.shape)
    D = d1 * d2
    P = len(panels)
    code = panel_code(panels)
    out_elem = _ELEM[out_dtype]
    frame_bytes = D * P * out_dtype.itemsize
    ex = Expander(ctx, pmd, dv, tabs, xt)

    if dest.kind == "device":
        sink = _DeviceSink(dest.target, frame_bytes)
    else:
        sink = _HostSink(ctx, dest, frame_bytes, (d1, P * d2), out_dtype, max(1, min(T, EXPORT_BLOCK)))
    walk, count = block_walk(plan, D), itertools.count()

    def consume(batch, elem, b0, n):
        for c0, m, yp in walk(batch, b0):
            ex.coefficients(c0, m)
            k = next(count)
            ex.expand(m, P, code, yp, elem, out=C.c_void_p(sink.dst(k, c0)), out_elem=out_elem)
            sink.done(k, c0, m)

    try:
        read_batches(ctx, movie, [(b0, b1) for b0, b1, _ in plan], frame_batch_size, num_workers, consume)
        sink.finish()
        ctx.sync()
    except BaseException:
        sink.abort()
        raise
