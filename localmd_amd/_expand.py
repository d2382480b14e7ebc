"""
The second half of the movie-pass scaffold: one 1024-frame block of the denoised and / or residual movie, rebuilt on the
device.  export_movie, regressor_maps (correlation), summary_images, quantile_images, superpixels and the two passes of
the rolling baseline (baseline.py) all do, per block,

    C = (R s) Vt[:, block]                       pmd_gemm, n_cols x 1024, leading dimension 1024
    frames = mean + std * (U C), y - that, y     pmd_group_expand (csrc/expand_fused.hip), panels side by side

and differ only in where the frames go.  The Expander holds what that takes on the device; the panel code, the layout
of a block of several panels and the device bytes are here with it.

The five consumers that turn the raw / denoised / residual movie into per-pixel state (summary_images, quantile_images,
regressor_maps, superpixels, the knots of the rolling baseline) also share their prologue and their walk.  KindPlan is
the host half: the shape, the block plan, the source's facts and the expand tables, built once per call before any
device work, and ``facts(dv)``, the keywords every ``*_device_bytes`` of the five takes.  KindBlocks is the device
half: the one Expander and the only walk, ``run(each, batch=...)``, which hands every block's raw frames in place and
its expanded panels to the caller's kernel.  Reading the movie, the block plan and the walk over a batch's blocks are
the first half, _stream.  No helper knows its caller.
"""
import numpy as np

from ._stream import (BLOCK, VtBlocks, block_plan, block_walk, factor_bytes, mean_std, read_batches, scaled_r,
                      source_info, upload_f32)

EXPORT_PATCH = 64       # pixels per patch of pmd_group_expand
ENTRY_FIELDS = 4        # {a_off, p64, r, c_row0}
_PANEL_CODE = {"raw": 0, "denoised": 1, "residual": 2}


def panel_code(panels):
    """The panels of a frame, left to right, as pmd_group_expand takes them: two bits each, the first panel lowest."""
    code = 0
    for j, k in enumerate(panels):
        code |= _PANEL_CODE[k] << (2 * j)
    return code


# ---- a block of P panels --------------------------------------------------------------------------------------------
# Frame f of an expanded block holds its P panels side by side, pixel (i, j) of panel p at i P d2 + p d2 + j.  A kernel
# that works pixel by pixel takes the block as a batch of P D "pixels"; what it needs or leaves per pixel is in the same
# (d1, P, d2) order.
def interleave(vectors, d1, d2):
    """(P D,): the P per-panel (D,) vectors (C pixel order) in the pixel order of an expanded block."""
    return np.stack([np.asarray(v).reshape(d1, d2) for v in vectors], axis=1).reshape(-1)


def split_panels(a, d1, P, d2):
    """The P contiguous per-panel (..., D) arrays of ``a``, whose last axis is P D in the pixel order of an expanded
    block."""
    lead = a.shape[:-1]
    v = a.reshape(lead + (d1, P, d2))
    return [np.ascontiguousarray(v[..., j, :]).reshape(lead + (d1 * d2,)) for j in range(P)]


def expander_bytes(*, D, n_cols, rank, n_entries, n_a, n_patches, factors_on_device, stats=True, own_ct=True,
                   block_panels=0):
    """Device bytes an Expander holds: the tables, the mean and std images (``stats``: left to a caller that counts
    them itself), one block of Vt columns and R s unless the PMDArray already holds it on the device, the coefficient
    block (``own_ct``) and the expanded block of ``block_panels`` panels."""
    need = 8 * (n_patches + 1) + n_entries * (8 * ENTRY_FIELDS + 4 * EXPORT_PATCH) + 4 * n_a
    need += factor_bytes(n_cols, rank, factors_on_device) + (2 * 4 * D if stats else 0)
    return need + (4 * n_cols * BLOCK if own_ct else 0) + 4 * block_panels * BLOCK * D


class Expander:
    """What one block's expansion takes on the device: the tables of pmd_group_expand (export.expand_tables_for), the
    mean and std images, R s, the Vt columns of the block and the coefficient block ``ct`` (``own_ct``; zero, and left
    so, without a product), and with ``block_panels`` = P > 0 the expanded block ``block`` (BLOCK x P D fp32).
    ``active``: U has columns and entries; ``product``: and the decomposition has rank, so there is a C to form."""

    def __init__(self, ctx, pmd, dv, tabs, xt, *, own_ct=True, block_panels=0):
        import torch

        dev, f32 = ctx.device, {"dtype": torch.float32, "device": ctx.device}
        self.ctx = ctx
        _, self.d1, self.d2 = (int(x) for x in pmd.shape)
        self.n_cols, self.rank = (int(x) for x in pmd.r.shape)
        self.n_patches, self.n_ent = int(xt["n_patches"]), len(xt["entries"])
        self.patch_ptr = torch.from_numpy(xt["patch_ptr"]).to(dev)
        self.entries = torch.from_numpy(np.ascontiguousarray(xt["entries"]).reshape(-1)).to(dev) if self.n_ent else None
        self.qmap = torch.from_numpy(xt["qmap"]).to(dev) if self.n_ent else None
        self.A = upload_f32(ctx, tabs["a"]) if self.n_ent else None
        self.mean, self.std = mean_std(ctx, pmd)
        self.active = self.n_cols > 0 and self.n_ent > 0
        self.product = self.active and self.rank > 0
        self.rs = scaled_r(ctx, pmd, dv) if self.product else None
        self.vt = VtBlocks(ctx, pmd, dv) if self.product else None
        self.ct = torch.zeros((self.n_cols, BLOCK), **f32) if self.active and own_ct else None
        self.block = torch.empty((BLOCK, block_panels * self.d1 * self.d2), **f32) if block_panels else None

    def coefficients(self, c0, m):
        """ct[:, :m] = (R s) Vt[:, c0:c0 + m]; nothing without a product."""
        from ._lib import ptr

        if self.product:
            self.vt.load(c0, m)
            self.ctx.call("pmd_gemm", 0, 0, self.n_cols, m, self.rank, 1.0, ptr(self.rs), self.rank, ptr(self.vt.buf),
                          BLOCK, 0.0, ptr(self.ct), BLOCK)

    def expand(self, n, n_panels, code, yp, elem, *, out=None, out_elem=0, coeff=None, ldc=BLOCK, mean=None):
        """n frames of ``n_panels`` side-by-side panels (``code``: panel_code) of element type ``out_elem`` at the
        device pointer ``out`` (default: the own fp32 block), from the coefficients ``ct`` (or ``coeff``, n_cols x ldc,
        column f = frame f) and the movie frames at ``yp`` of element type ``elem`` (None without a movie); ``mean``
        replaces the mean image."""
        from ._lib import ptr

        self.ctx.call("pmd_group_expand", ptr(self.ct if coeff is None else coeff), int(ldc), int(n), self.d1, self.d2,
                      ptr(self.mean if mean is None else mean), ptr(self.std), self.n_patches, ptr(self.patch_ptr),
                      self.n_ent, ptr(self.entries), ptr(self.qmap), ptr(self.A), yp, int(elem), self.d1 * self.d2,
                      int(n_panels), int(code), ptr(self.block) if out is None else out, int(out_elem))


# ---- the per-pixel consumers: one plan, one walk --------------------------------------------------------------------
class KindPlan:
    """The host half of a pass that turns the raw (``raw``) and / or expanded (``panels``: "denoised", "residual") movie
    into per-pixel state; no device work.  ``T, d1, d2, D``; ``plan`` (block_plan) and ``nb``, the frames of its first
    batch; ``on_device, esize`` (source_info of a ``movie`` that is given, else (False, 4)); ``n_cols, rank``;
    ``reads_movie``, and ``movie``, None unless it is read; ``tabs, xt``, the tables of pmd_group_expand, built once and
    only for panels or ``tables=True`` (None otherwise).  A decomposition of no frames has no blocks and builds no
    tables: what that means is the caller's to say."""

    def __init__(self, pmd, movie, *, raw, panels, frame_batch_size, tables=False):
        self.T, self.d1, self.d2 = (int(x) for x in pmd.shape)
        self.D = self.d1 * self.d2
        self.raw, self.panels = bool(raw), tuple(panels)
        self.reads_movie = self.raw or "residual" in self.panels
        self.on_device, self.esize = source_info(movie, pmd.shape) if movie is not None else (False, 4)
        self.movie = movie if self.reads_movie else None
        self.frame_batch_size = frame_batch_size
        self.plan = block_plan(self.T, frame_batch_size) if self.T else []
        self.nb = self.plan[0][1] - self.plan[0][0] if self.plan else 0
        self.n_cols, self.rank = (int(x) for x in pmd.r.shape)
        self.tabs = self.xt = None
        if self.T and (self.panels or tables):
            from .export import expand_tables_for

            self.tabs, self.xt = expand_tables_for(pmd)

    def facts(self, dv):
        """The keywords every ``*_device_bytes`` of the per-pixel consumers takes; ``dv``: device_context's."""
        tabs, xt = self.tabs, self.xt
        return dict(D=self.D, nb=self.nb, esize=self.esize, n_cols=self.n_cols, rank=self.rank,
                    n_entries=len(xt["entries"]) if xt else 0, n_a=int(tabs["a"].size) if tabs else 0,
                    n_patches=int(xt["n_patches"]) if xt else 0, host_source=not self.on_device,
                    n_batches=len(self.plan), factors_on_device=dv is not None)


class KindBlocks:
    """The device half: the Expander of the plan's panels as ``ex`` (None when the plan built no tables; ``own_ct``: see
    Expander) and the walk over the plan's blocks."""

    def __init__(self, ctx, pmd, dv, plan, num_workers, *, own_ct=True):
        self.ctx, self.plan, self.num_workers = ctx, plan, num_workers
        self.P, self.code = len(plan.panels), panel_code(plan.panels)
        self.ex = None
        if plan.xt is not None:
            self.ex = Expander(ctx, pmd, dv, plan.tabs, plan.xt, own_ct=own_ct, block_panels=self.P)

    def run(self, each, *, batch=None, before=None, read_movie=True):
        """One pass in frame order.  ``batch(ptr, elem, b0, n)``, when given, gets every batch of the movie whole, before
        its blocks (no call without a movie).  For every reconstruction block the panels are expanded into ``ex.block``
        and ``each(c0, m, yp, elem, xp)`` is called: yp the block's raw frames in place in the batch, of element type
        elem (None, 0 without a movie), xp the expanded block (None without panels).  ``before(c0, m, yp, elem)``, when
        given, is called ahead of the block's product and expansion: the place of a step that makes the host wait for
        the stream (a copy from pageable memory), which there waits for the block before and not for this block's
        expansion.  ``read_movie=False``: the same blocks, no movie."""
        from ._lib import ptr

        kp, ex, P, code = self.plan, self.ex, self.P, self.code
        walk = block_walk(kp.plan, kp.D)
        xp = ptr(ex.block) if P else None

        def consume(frames, elem, b0, n):
            if batch is not None and frames is not None:
                batch(ptr(frames), elem, b0, n)
            for c0, m, yp in walk(frames, b0):
                if before is not None:
                    before(c0, m, yp, elem)
                if P:
                    ex.coefficients(c0, m)
                    ex.expand(m, P, code, yp, elem)
                each(c0, m, yp, elem, xp)

        read_batches(self.ctx, kp.movie if read_movie else None, [(b0, b1) for b0, b1, _ in kp.plan],
                     kp.frame_batch_size, self.num_workers, consume)
