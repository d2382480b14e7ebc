"""
Summary images of a movie: per-pixel extrema and moment images, the pictures cell finding, ROI drawing and quality
control start from.

``summary_images(pmd, movie, kinds=..., stats=...)`` returns (d1, d2) images of the raw movie, the denoised movie
``mean + std * (U R diag(s) Vt)`` and their difference: the mean, std, skewness and excess kurtosis over the frames, the
minimum and maximum with the frames that attain them, and the peak-to-noise ratio.  None of them is linear in the movie,
so every pixel of every frame is looked at, once:

* raw: every 1024-frame block of every batch, in the movie's own dtype and from the batch in place, goes through
  ``pmd_pixel_stats_accumulate`` (csrc/stats.hip), which keeps the running extrema (fp32, with int32 frame numbers) and
  the four power sums about a centring vector (fp32 within a block, fp64 across blocks) on the device.
* denoised and residual: the block is expanded on the device by _expand.Expander, as in export_movie (``pmd_gemm`` of
  R s with the Vt block, ``pmd_group_expand``), and the same kernel takes the expanded buffer as a batch of P D pixels.
* the host finishes in float64 (finish_moments, finish_pnr) and rounds every image once.

Blocks start on multiples of 1024 whatever the batch size, so every output bit is the same for every batching and
source.  The movie is read once through the scaffold of _stream; device memory does not grow with its length.
"""
import numpy as np

from ._expand import KindBlocks, KindPlan, expander_bytes, interleave, split_panels
from ._movie import _device_free_bytes
from ._stream import batch_buffer_bytes, check_fit, check_pmd, device_context, name_tuple, upload_f32
from .maps import GAMMA, KINDS, centring_vector

STATS = ("mean", "std", "min", "max", "argmin", "argmax", "skewness", "kurtosis", "pnr")
_EXT_STATS = ("min", "max", "argmin", "argmax", "pnr")             # what needs the running extrema,
_ARG_STATS = ("argmin", "argmax")                                  # their frame numbers,
_MOM_STATS = ("mean", "std", "skewness", "kurtosis", "pnr")        # the power sums
MAX_BIN = 1024


class Summary:
    """Result of summary_images: ``denoised``, ``raw``, ``residual`` (each a dict stat -> (d1, d2) image, or None when
    not asked for), ``stats`` (the names asked for) and ``temporal_bin``."""

    def __init__(self, denoised=None, raw=None, residual=None, stats=(), temporal_bin=1):
        self.denoised, self.raw, self.residual = denoised, raw, residual
        self.stats, self.temporal_bin = tuple(stats), int(temporal_bin)

    def __repr__(self):
        have = [k for k in KINDS if getattr(self, k) is not None]
        return "Summary({}; {}; temporal_bin={})".format(", ".join(have), ", ".join(self.stats), self.temporal_bin)


# ---- host-side finishing (no device work) --------------------------------------------------------------------------
def finish_moments(S, T, centre):
    """{"mean", "std", "skewness", "kurtosis"} in float64 from the power sums ``S[p] = sum_t (y_t - centre)^(p + 1)``
    ((4, N) float64) of T frames: with d = S1 / T the mean is centre + d and the central moments are
    m2 = S2 / T - d^2, m3 = S3 / T - 3 d S2 / T + 2 d^3, m4 = S4 / T - 4 d S3 / T + 6 d^2 S2 / T - 3 d^4; std = sqrt(m2)
    (population, ddof = 0), skewness = m3 / m2^1.5, kurtosis = m4 / m2^2 - 3.  The block sums behind S are fp32 chains,
    so a variance with T m2 <= 3 GAMMA S2 cannot be told from that of a constant pixel (maps._pearson) and counts as
    zero: std, skewness and kurtosis are then 0."""
    S = np.asarray(S, dtype=np.float64)
    T = float(T)
    a1, a2, a3, a4 = (S[p] / T for p in range(4))
    m2 = a2 - a1 * a1
    m3 = a3 - 3.0 * a1 * a2 + 2.0 * a1 ** 3
    m4 = a4 - 4.0 * a1 * a3 + 6.0 * a1 * a1 * a2 - 3.0 * a1 ** 4
    ok = T * m2 > 3.0 * GAMMA * S[1]
    v = np.where(ok, m2, 1.0)
    with np.errstate(invalid="ignore", divide="ignore"):     # non-finite sums (a NaN frame) stay non-finite
        return {"mean": np.asarray(centre, dtype=np.float64) + a1,
                "std": np.where(ok, np.sqrt(v), 0.0),
                "skewness": np.where(ok, m3 / v ** 1.5, 0.0),
                "kurtosis": np.where(ok, m4 / (v * v) - 3.0, 0.0)}


def finish_pnr(peak, mean, noise):
    """(peak - mean) / noise in float64, rounded once to float32; 0 where ``noise`` is not finite or not positive."""
    noise = np.asarray(noise, dtype=np.float64)
    ok = np.isfinite(noise) & (noise > 0)
    with np.errstate(invalid="ignore"):
        r = (np.asarray(peak, dtype=np.float64) - np.asarray(mean, dtype=np.float64)) / np.where(ok, noise, 1.0)
    return np.where(ok, r, 0.0).astype(np.float32)


def summary_device_bytes(*, D, nb, esize, n_raw, n_expand, need_ext, need_arg, need_mom, n_cols, rank, n_entries, n_a,
                         n_patches, needs_movie, host_source, n_batches, factors_on_device):
    """Device bytes summary_images holds on a movie of D pixels read in batches of nb frames; no term grows with the
    movie's length.  The state of every kind (8 bytes of extrema, 8 of frame numbers and 32 of power sums per pixel, as
    far as the stats need them) with its centring vector, the batch buffers, and for the n_expand expanded panels one
    expanded block with the coefficient block and tables of pmd_group_expand, the mean and std images, one block of Vt
    columns, and R s unless the PMDArray already holds it on the device."""
    per_px = 8 * int(bool(need_ext)) + 8 * int(bool(need_arg)) + 32 * int(bool(need_mom)) + 4
    need = per_px * (n_raw + n_expand) * D
    if needs_movie:
        need += batch_buffer_bytes(nb, D, esize, host_source, n_batches)
    if n_expand:
        need += expander_bytes(D=D, n_cols=n_cols, rank=rank, n_entries=n_entries, n_a=n_a, n_patches=n_patches,
                               factors_on_device=factors_on_device, block_panels=n_expand)
    return need + (1 << 20)     # the allocator's rounding of the small arrays


def _check_bin(temporal_bin):
    ok = isinstance(temporal_bin, (int, np.integer)) and not isinstance(temporal_bin, (bool, np.bool_))
    if not ok or not 1 <= int(temporal_bin) <= MAX_BIN or int(temporal_bin) & (int(temporal_bin) - 1):
        raise ValueError("temporal_bin must be a power of two from 1 to {}, got {!r}".format(MAX_BIN, temporal_bin))
    return int(temporal_bin)


# ---- public entry point --------------------------------------------------------------------------------------------
def summary_images(pmd, movie=None, *, kinds="denoised", stats=("mean", "std", "max"), temporal_bin=1,
                   frame_batch_size=10000, num_workers=0, device=None, ctx=None):
    """Per-pixel summary images: ``kinds`` is any non-empty subset of "denoised" (of ``mean_img + var_img * (U R diag(s)
    Vt)``), "raw" (of ``movie``) and "residual" (of raw - denoised); ``stats`` any non-empty subset of STATS.  Returns a
    Summary whose ``denoised`` / ``raw`` / ``residual`` are dicts stat -> (d1, d2) image in natural orientation (None
    for kinds not asked for); "argmin" and "argmax" are int32 frame numbers, every other stat is float32.

    * "mean", "std": population moments over the frames (ddof = 0); "skewness" = m3 / m2^1.5 and "kurtosis" =
      m4 / m2^2 - 3 from the central moments.  The device forms the power sums of a 1024-frame block in fp32 about a
      centring vector (raw: maps.centring_vector, denoised: the mean image, residual: 0), so a variance at or below
      3 GAMMA sum z^2 (GAMMA = 1032 * 2^-24) counts as zero and std, skewness and kurtosis are 0 there: every constant
      pixel (see regressor_maps).
    * "min", "max": the extrema over the frames, exactly; "argmin", "argmax": the first frame that attains them.
    * "pnr": (max - mean) / noise with the decomposition's noise std image (``pmd.var_img``), computed in float64 and
      rounded once; 0 where the noise is not finite or not positive.

    ``temporal_bin`` (a power of two from 1 to 1024): the extrema ("min", "max", "argmin", "argmax" and the max inside
    "pnr") are taken over the means of consecutive bins of that many frames, which start at frame 0 (a last bin with
    fewer frames is averaged over the frames it has); "argmin" and "argmax" then name the bin's first frame.  The
    moments ("mean", "std", "skewness", "kurtosis" and the mean inside "pnr") are always over frames, whatever
    temporal_bin is.

    ``movie`` (of ``pmd.shape``; not needed, and never touched, when only "denoised" is asked for): the sources of
    regressor_maps, read once in ``frame_batch_size`` batches, uint16 / int16 in their own dtype.  After
    ``pmd.to_device()`` its context and uploaded factors are reused.  Every image has the same bits for every
    frame_batch_size and source, for every order and subset of kinds and stats.  Argument errors are raised before any
    device work and before the movie is read; a decomposition of no frames has no extrema and raises ValueError."""
    check_pmd(pmd)
    kinds = name_tuple(kinds, KINDS, "kind", "kinds")
    stats = name_tuple(stats, STATS, "stat", "stats")
    temporal_bin = _check_bin(temporal_bin)
    if kinds != ("denoised",) and movie is None:
        raise ValueError("kinds {} need the movie: pass movie=".format(kinds))
    kp = KindPlan(pmd, movie, raw="raw" in kinds, panels=tuple(k for k in ("denoised", "residual") if k in kinds),
                  frame_batch_size=frame_batch_size)
    if kp.T == 0:
        raise ValueError("the decomposition has no frames: their extrema do not exist")
    need = tuple(any(s in names for s in stats) for names in (_EXT_STATS, _ARG_STATS, _MOM_STATS))

    with device_context(pmd, device, ctx) as (ctx, dv):
        nbytes = summary_device_bytes(**kp.facts(dv), n_raw=int(kp.raw), n_expand=len(kp.panels), need_ext=need[0],
                                      need_arg=need[1], need_mom=need[2], needs_movie=kp.reads_movie)
        check_fit("summary_images", nbytes, _device_free_bytes(ctx.device))
        out = _summary(ctx, pmd, KindBlocks(ctx, pmd, dv, kp, num_workers), stats, need, temporal_bin)
    return Summary(stats=stats, temporal_bin=temporal_bin, **{k: out[k] for k in kinds})


class _State:
    """The running state of pmd_pixel_stats_accumulate for N pixels on the device: ext [2][N] fp32 (+inf, -inf), arg
    [2][N] int32 (-1), mom [4][N] fp64 (0), each only when needed, and the centring vector of the moments."""

    def __init__(self, ctx, N, need, centre):
        import torch

        dev = ctx.device
        self.N = N
        self.ext = self.arg = self.mom = self.centre = None
        if need[0]:
            self.ext = torch.empty((2, N), dtype=torch.float32, device=dev)
            self.ext[0].fill_(float("inf"))
            self.ext[1].fill_(float("-inf"))
        if need[1]:
            self.arg = torch.full((2, N), -1, dtype=torch.int32, device=dev)
        if need[2]:
            self.mom = torch.zeros((4, N), dtype=torch.float64, device=dev)
            self.centre = upload_f32(ctx, centre)

    def accumulate(self, ctx, Y, elem, n, f0, temporal_bin):
        from ._lib import ptr

        ctx.call("pmd_pixel_stats_accumulate", Y, int(elem), self.N, int(n), self.N, int(f0), int(temporal_bin),
                 ptr(self.centre), ptr(self.ext), ptr(self.arg), ptr(self.mom))

    def host(self):
        return tuple(None if t is None else t.cpu().numpy() for t in (self.ext, self.arg, self.mom))


def _summary(ctx, pmd, blocks, stats, need, temporal_bin):
    kp = blocks.plan
    T, d1, d2, D, do_raw, panels = kp.T, kp.d1, kp.d2, kp.D, kp.raw, kp.panels
    P = len(panels)
    mean32 = np.asarray(pmd.mean_img, dtype=np.float32).reshape(-1)
    centre32 = centring_vector(pmd)
    raw = _State(ctx, D, need, centre32) if do_raw else None
    if P:
        # the kernel takes the expanded block as a batch of P D "pixels" whose centring vector is the mean image under
        # the denoised panel and 0 under the residual panel
        centres = {"denoised": mean32, "residual": np.zeros(D, np.float32)}
        expanded = _State(ctx, P * D, need, interleave([centres[k] for k in panels], d1, d2))

    def each(c0, m, yp, elem, xp):
        if do_raw:
            raw.accumulate(ctx, yp, elem, m, c0, temporal_bin)
        if P:
            expanded.accumulate(ctx, xp, 0, m, c0, temporal_bin)

    blocks.run(each)
    ctx.sync()

    noise = np.asarray(pmd.var_img, dtype=np.float64).reshape(-1)      # the std image, see _stream.mean_std
    out = {}
    if do_raw:
        out["raw"] = _finish(stats, raw.host(), T, centre32, noise, (d1, d2))
    if P:
        state = [None if a is None else split_panels(a, d1, P, d2) for a in expanded.host()]
        for j, k in enumerate(panels):
            one = tuple(None if a is None else a[j] for a in state)
            out[k] = _finish(stats, one, T, centres[k], noise, (d1, d2))
    return out


def _finish(stats, state, T, centre32, noise, shape):
    """The images ``stats`` of one kind from its device state (ext, arg, mom over the pixels in C order)."""
    ext, arg, mom = state
    mo = finish_moments(mom, T, centre32.astype(np.float64)) if mom is not None else None
    img = {}
    for s in stats:
        if s in ("min", "max"):
            a = ext[0 if s == "min" else 1]
        elif s in _ARG_STATS:
            a = arg[0 if s == "argmin" else 1]
        elif s == "pnr":
            a = finish_pnr(ext[1], mo["mean"], noise)
        else:
            a = mo[s].astype(np.float32)
        img[s] = np.ascontiguousarray(a).reshape(shape)
    return img
