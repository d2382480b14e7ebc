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
block those of _expand.Expander, shared with regressor_maps, summary_images and quantile_images.  The destinations, the
sinks (host destinations get each block through a ring of two device and two page-locked buffers while a writer thread
puts the frames into the file or array) and the scaffold that opens, finishes and aborts them are _sink's, shared with
dff_movie and the two registrations; what is left here is the tables, the argument checks and the block's two calls.
Device memory and host memory do not grow with the movie's length.
"""
import numpy as np

from ._expand import ENTRY_FIELDS, EXPORT_PATCH, _PANEL_CODE, Expander, expander_bytes, panel_code  # noqa: F401
from ._movie import _ELEM, _device_free_bytes
from ._sink import HOST_SLOTS, _destination, check_bigtiff, device_index, movie_pass  # noqa: F401
from ._stream import BLOCK as EXPORT_BLOCK, block_plan as export_plan
from ._stream import batch_buffer_bytes, check_fit, check_pmd, device_context, each_block, name_tuple, source_info
from .projection import MAX_ROWS, P_MAX, ROW_PAD, _pad, tables_for

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
    check_pmd(pmd)
    panels = name_tuple(panels, PANELS, "panel", "panels")
    out_dtype = _out_dtype(dtype)
    check_bigtiff(bigtiff)
    T, d1, d2 = (int(x) for x in pmd.shape)
    D = d1 * d2
    needs_movie = any(p != "denoised" for p in panels)
    if needs_movie and movie is None:
        raise ValueError("panels {} need the movie: pass movie=".format(tuple(p for p in panels if p != "denoised")))
    on_device, esize = source_info(movie, pmd.shape) if movie is not None else (False, 4)
    dev_index = device_index(pmd, device, ctx)
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
        ex = Expander(ctx, pmd, dv, tabs, xt)
        P, code, out_elem = len(panels), panel_code(panels), _ELEM[out_dtype]

        def write(c0, m, yp, elem, to):
            ex.coefficients(c0, m)
            ex.expand(m, P, code, yp, elem, out=to, out_elem=out_elem)

        return movie_pass(ctx, dest, (d1, P * d2), out_dtype, max(1, min(T, EXPORT_BLOCK)),
                          each_block(ctx, movie if needs_movie else None, plan, D, frame_batch_size, num_workers), write)
