"""
The second half of the movie-pass scaffold: one 1024-frame block of the denoised and / or residual movie, rebuilt on the
device.  export_movie, regressor_maps (correlation), summary_images, quantile_images and the two passes of the rolling
baseline (baseline.py) all do, per block,

    C = (R s) Vt[:, block]                       pmd_gemm, n_cols x 1024, leading dimension 1024
    frames = mean + std * (U C), y - that, y     pmd_group_expand (csrc/expand_fused.hip), panels side by side

and differ only in where the frames go.  The Expander holds what that takes on the device; the panel code, the layout
of a block of several panels and the device bytes are here with it.  Reading the movie, the block plan and the walk over
a batch's blocks are the first half, _stream.  No helper knows its caller.
"""
import numpy as np

from ._stream import BLOCK, VtBlocks, factor_bytes, mean_std, scaled_r, upload_f32

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
