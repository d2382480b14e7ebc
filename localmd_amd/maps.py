"""
Per-pixel maps of a movie against time courses: ``M = Y X^T``, the transposed product of extract_traces (masks in, time
courses out; here time courses in, images out).

``regressor_maps(pmd, regressors, movie, kinds=..., stat=...)`` returns (K, d1, d2) float32 images for K time courses
``X`` (K x T), for the raw movie, the denoised movie ``mean + std * (U R diag(s) Vt)`` and their difference:

* ``stat="sum"``: ``M[k, p] = sum_t x_k[t] y_p[t]``; ``"mean"``: the sum divided by ``sum_t x_k[t]`` (with the rows of
  event_regressors an event-triggered average); ``"correlation"``: the Pearson correlation of ``x_k`` with ``y_p``.
* raw: every 1024-frame block of every batch, in the movie's own dtype, goes through ``pmd_regress_accumulate``
  (csrc/regress.hip): fp32 matrix-core products of a block, centred by the decomposition's mean image on a dyadic grid
  (centring_vector), added into fp64 accumulators on the device; the host finishes in fp64
  (``sum x y = acc + centre sum x``) and rounds once.
* denoised sums never touch a pixel per frame: ``G = Vt X^T`` (rank x K) is accumulated over the blocks of Vt in fp64,
  ``Cm = (R diag(s)) G`` is K pseudo-frames of coefficients and one ``pmd_group_expand`` call turns them into images.
* for the correlation the denoised and residual blocks are expanded on the device (the export path) and go through the
  same kernel, which also forms ``sum z`` and ``sum z^2`` of every pixel.

Blocks start on multiples of 1024 whatever the batch size, so every output bit is the same for every batching and
source.  The movie is read once through the scaffold of _stream; device memory does not grow with its length.
"""
import numpy as np

from ._expand import KindBlocks, KindPlan, expander_bytes, interleave, panel_code, split_panels
from ._movie import _device_free_bytes
from ._stream import BLOCK, batch_buffer_bytes, check_fit, check_pmd, device_context, name_tuple, upload_f32

KINDS = ("denoised", "raw", "residual")
STATS = ("sum", "mean", "correlation")
GAMMA = (BLOCK + 8) * 2.0 ** -24                  # forward error of one block's fp32 sums, relative to the sum of magnitudes


class Maps:
    """Result of regressor_maps: ``denoised``, ``raw``, ``residual`` ((K, d1, d2) float32, or None when not asked
    for)."""

    def __init__(self, denoised=None, raw=None, residual=None):
        self.denoised, self.raw, self.residual = denoised, raw, residual

    def __repr__(self):
        have = [k for k in KINDS if getattr(self, k) is not None]
        return "Maps({} regressors, {})".format(len(getattr(self, have[0])) if have else 0, ", ".join(have))


# ---- argument checks and host-side preparation (no device work) ----------------------------------------------------
def event_regressors(T, events, lags):
    """(len(lags), T) float64: row l has weight 1 / n_l at every frame ``e + lags[l]`` that lies in [0, T) (n_l of the
    events do), 0 elsewhere.  With ``stat="mean"`` (or "sum": the rows sum to 1) the map of row l is the average frame
    ``lags[l]`` frames after an event.  Events that coincide at a lag count as often as they occur."""
    T = int(T)
    ev = np.asarray(events).reshape(-1)
    lg = np.asarray(lags).reshape(-1)
    if T < 1:
        raise ValueError("T must be positive, got {}".format(T))
    if ev.size == 0 or lg.size == 0:
        raise ValueError("events and lags must not be empty")
    if ev.dtype.kind not in "iu" or lg.dtype.kind not in "iu":
        raise ValueError("events and lags must be integers (frame numbers), got {} and {}".format(ev.dtype, lg.dtype))
    out = np.zeros((lg.size, T), dtype=np.float64)
    for row, lag in enumerate(lg.astype(np.int64)):
        t = ev.astype(np.int64) + lag
        t = t[(t >= 0) & (t < T)]
        if t.size == 0:
            raise ValueError("lag {}: no event lands inside the {} frames".format(int(lag), T))
        np.add.at(out[row], t, 1.0 / t.size)
    return out


def prepare_regressors(regressors, T):
    """``regressors`` ((K, T), or (T,) for K = 1) as a finite (K, T) float64 array."""
    x = np.asarray(regressors)
    if x.dtype.kind not in "biuf":
        raise ValueError("regressors must be real numbers, got {}".format(x.dtype))
    if x.ndim == 1:
        x = x[None, :]
    if x.ndim != 2:
        raise ValueError("regressors must be shaped (K, T) or (T,), got {}".format(x.shape))
    if x.shape[1] != int(T):
        raise ValueError("regressors have {} frames, the decomposition {}".format(x.shape[1], int(T)))
    if x.shape[0] == 0:
        raise ValueError("regressors hold no time course (K = 0)")
    x = np.ascontiguousarray(x, dtype=np.float64)
    if not np.all(np.isfinite(x)):
        raise ValueError("regressors hold non-finite values")
    with np.errstate(over="ignore"):
        if not np.all(np.isfinite(x.astype(np.float32))):
            raise ValueError("regressors hold values outside the float32 range")
    return x


def normalized_regressors(x64):
    """Every row of ``x64`` centred and scaled to unit norm in float64 (a row without variance becomes zeros), so that
    the fp32 copy the device works with loses nothing to a trace's offset."""
    xc = x64 - x64.mean(axis=1, keepdims=True)
    xc -= xc.mean(axis=1, keepdims=True)         # the second pass removes the rounding left by a large offset
    norm = np.sqrt((xc * xc).sum(axis=1, keepdims=True))
    scale = np.abs(x64).max(axis=1, keepdims=True)
    flat = norm <= 1e-14 * np.sqrt(x64.shape[1]) * scale      # constant up to the rounding of the centring
    return np.where(flat, 0.0, xc / np.where(flat, 1.0, norm))


def centring_vector(pmd):
    """(D,) float32, C pixel order: what the raw pixels are centred by on the device, the mean image rounded to a
    multiple of q = 2^floor(log2(std / 8)) of the pixel's noise std.  It stays within std / 16 of the mean, so the fp32
    sums run at the size of the fluctuations, and it lies on a dyadic grid: the centred values of an integer movie are
    multiples of min(q, 1), so its block sums are exact where they stay below 2^24 q.  A pixel without a usable std
    (0, non-finite, or below 2^-20 of the mean) is centred by the mean itself."""
    mean = np.asarray(pmd.mean_img, dtype=np.float32).reshape(-1).astype(np.float64)
    std = np.asarray(pmd.var_img, dtype=np.float32).reshape(-1).astype(np.float64)     # the std image, see _stream.mean_std
    ok = np.isfinite(std) & (std > 0) & np.isfinite(mean) & (np.abs(mean) < 2.0 ** 20 * std)
    q = np.exp2(np.floor(np.log2(np.where(ok, std, 8.0) / 8.0)))
    return np.where(ok, np.rint(mean / q) * q, mean).astype(np.float32)


def maps_device_bytes(*, D, nb, esize, K, n_acc, n_expand, n_cols, rank, n_entries, n_a, n_patches, needs_movie,
                      host_source, n_batches, factors_on_device, factor_sums):
    """Device bytes regressor_maps holds for K regressors on a movie of D pixels read in batches of nb frames; no term
    grows with the movie's length.  The fp64 accumulators (K x D for each of the n_acc kernel-accumulated kinds) and
    their moment vectors, the batch buffers, one block of regressors, one expanded block per expanded panel with the
    coefficient block and tables of pmd_group_expand, one block of Vt columns, and R s unless the PMDArray already holds
    it on the device; ``factor_sums``: the denoised sums from the factors (G, Cm and their K images)."""
    need = 8 * n_acc * (K + 2) * D + 4 * K * BLOCK + 2 * 4 * D
    if needs_movie:
        need += batch_buffer_bytes(nb, D, esize, host_source, n_batches)
    if n_expand or factor_sums:     # the mean and std images are counted above, whatever runs
        need += expander_bytes(D=D, n_cols=n_cols, rank=rank, n_entries=n_entries, n_a=n_a, n_patches=n_patches,
                               factors_on_device=factors_on_device, stats=False, own_ct=bool(n_expand),
                               block_panels=n_expand)
    if n_expand:
        need += 4 * n_expand * D
    if factor_sums:
        need += 16 * rank * K + 4 * n_cols * K + 4 * K * D + 4 * D
    return need + (1 << 20)     # the allocator's rounding of the small arrays


# ---- public entry point --------------------------------------------------------------------------------------------
def regressor_maps(pmd, regressors, movie=None, *, kinds="denoised", stat="sum", frame_batch_size=10000, num_workers=0,
                   device=None, ctx=None):
    """Maps of the time courses ``regressors`` ((K, T) real, or (T,); the rows of extract_traces can be passed straight
    in): ``kinds`` is any non-empty subset of "denoised" (against ``mean_img + var_img * (U R diag(s) Vt)``), "raw"
    (against ``movie``) and "residual" (against raw - denoised).  ``stat``: "sum" (``sum_t x_k[t] y_p[t]``), "mean" (the
    sum divided by ``sum_t x_k[t]``) or "correlation" (Pearson, 0 where either side has no variance).  Returns a Maps
    object with (K, d1, d2) float32 images in natural orientation (None for kinds not asked for).  Under "sum" and
    "mean" the residual is raw - denoised of the returned values, element by element.

    Under "correlation" the device centres the raw pixels by the mean image rounded to a dyadic grid (centring_vector)
    and forms the sums of a 1024-frame block in fp32, so a pixel's variance is known to about 3 GAMMA sum z^2
    (GAMMA = 1032 * 2^-24) of its centred values z.  A variance at or below that floor counts as zero and the pixel's
    correlation is 0, not a noisy value: this is every constant pixel, and any pixel whose offset from the centring
    vector is more than about 73 times its own std (kappa = |z| / |z - mean z| > 1 / sqrt(3 GAMMA)), which happens when
    the movie passed in is not the one the decomposition's mean image was formed from.

    ``movie`` (of ``pmd.shape``; not needed, and never touched, when only denoised sums or means are asked for): NumPy
    arrays and memmaps, any lazy_data_loader (TiffArray included), CPU tensors (read once in ``frame_batch_size``
    batches through the pinned staging ring of the streamed decomposition, uint16 / int16 in their own dtype) and
    device tensors (sliced in place).  After ``pmd.to_device()`` its context and uploaded factors are reused.  Every
    map has the same bits for every frame_batch_size and source.  Argument errors are raised before any device work
    and before the movie is read."""
    check_pmd(pmd)
    kinds = name_tuple(kinds, KINDS, "kind", "kinds")
    if not isinstance(stat, str) or stat not in STATS:
        raise ValueError("unknown stat {!r}; choose from {}".format(stat, STATS))
    T, d1, d2 = (int(x) for x in pmd.shape)
    x64 = prepare_regressors(regressors, T)
    K = x64.shape[0]
    if stat == "mean":
        tot = x64.sum(axis=1)
        if np.any(tot == 0):
            raise ValueError("stat='mean': regressor {} sums to 0".format(int(np.argmax(tot == 0))))
    corr = stat == "correlation"
    movie_required = corr or kinds != ("denoised",)
    if movie_required and movie is None:
        raise ValueError("kinds {} with stat {!r} need the movie: pass movie=".format(kinds, stat))
    # what runs: the raw accumulation, the expanded panels (correlation only), the denoised sums from the factors
    do_raw = "raw" in kinds or (not corr and "residual" in kinds)
    panels = tuple(k for k in ("denoised", "residual") if k in kinds) if corr else ()
    factor_sums = not corr and ("denoised" in kinds or "residual" in kinds)
    kp = KindPlan(pmd, movie, raw=do_raw, panels=panels, frame_batch_size=frame_batch_size, tables=factor_sums)
    if T == 0:
        return Maps(**{k: np.zeros((K, d1, d2), dtype=np.float32) for k in kinds})

    with device_context(pmd, device, ctx) as (ctx, dv):
        need = maps_device_bytes(**kp.facts(dv), K=K, n_acc=int(do_raw) + len(panels), n_expand=len(panels),
                                 needs_movie=kp.reads_movie, factor_sums=factor_sums)
        check_fit("regressor_maps", need, _device_free_bytes(ctx.device))
        out = _maps(ctx, pmd, KindBlocks(ctx, pmd, dv, kp, num_workers, own_ct=bool(panels)), x64, kinds, stat,
                    factor_sums)
    return Maps(**{k: out[k].reshape(K, d1, d2) for k in kinds})


def _maps(ctx, pmd, blocks, x64, kinds, stat, factor_sums):
    import torch
    from ._lib import ptr

    kp, ex = blocks.plan, blocks.ex
    T, d1, d2, D, do_raw, panels = kp.T, kp.d1, kp.d2, kp.D, kp.raw, kp.panels
    dev = ctx.device
    K = x64.shape[0]
    corr = stat == "correlation"
    P = len(panels)
    xdev64 = normalized_regressors(x64) if corr else x64
    x32 = np.ascontiguousarray(xdev64, dtype=np.float32)              # what the device multiplies with
    x_host = torch.from_numpy(x32)
    xb = torch.zeros((K, BLOCK), dtype=torch.float32, device=dev)     # the regressors of one block
    mean32 = np.asarray(pmd.mean_img, dtype=np.float32).reshape(-1).astype(np.float64)
    centre32 = centring_vector(pmd)
    centre = upload_f32(ctx, centre32) if do_raw else None

    acc_raw = torch.zeros((K, D), dtype=torch.float64, device=dev) if do_raw else None
    mom_raw = torch.zeros(2 * D, dtype=torch.float64, device=dev) if do_raw and corr else None
    if P:
        # the kernel takes the expanded block as a batch of P D "pixels" whose centring vector is the mean image under
        # the denoised panel and 0 under the residual panel
        centres = {"denoised": mean32.astype(np.float32), "residual": np.zeros(D, np.float32)}
        shift = upload_f32(ctx, interleave([centres[k] for k in panels], d1, d2))
        acc_ex = torch.zeros((K, P * D), dtype=torch.float64, device=dev)
        mom_ex = torch.zeros(2 * P * D, dtype=torch.float64, device=dev)
    if factor_sums and ex.product:
        g64 = torch.zeros((ex.rank, K), dtype=torch.float64, device=dev)
        gb = torch.empty((ex.rank, K), dtype=torch.float32, device=dev)

    def before(c0, m, yp, elem):
        xb[:, :m].copy_(x_host[:, c0:c0 + m])             # a blocking copy from pageable memory, once per block
        if do_raw:
            ctx.call("pmd_regress_accumulate", yp, int(elem), D, m, D, ptr(centre), ptr(xb), BLOCK, K, ptr(acc_raw), D,
                     ptr(mom_raw))

    def each(c0, m, yp, elem, xp):
        if P:
            ctx.call("pmd_regress_accumulate", xp, 0, P * D, m, P * D, ptr(shift), ptr(xb), BLOCK, K, ptr(acc_ex), P * D,
                     ptr(mom_ex))
        if factor_sums and ex.product:
            # G += Vt[:, block] X[:, block]^T: every block product has the same shape; fp64 across the blocks
            ex.vt.load(c0, m)
            ctx.call("pmd_gemm", 0, 1, ex.rank, K, m, 1.0, ptr(ex.vt.buf), BLOCK, ptr(xb), BLOCK, 0.0, ptr(gb), K)
            g64.add_(gb)

    blocks.run(each, before=before)

    den_img = None
    if factor_sums:
        if ex.product:
            # Cm = (R s) G as K pseudo-frames of coefficients, expanded with a zero mean: std * (U Cm) in (K, d1, d2)
            cm = torch.empty((ex.n_cols, K), dtype=torch.float32, device=dev)
            g32 = g64.to(torch.float32)
            ctx.call("pmd_gemm", 0, 0, ex.n_cols, K, ex.rank, 1.0, ptr(ex.rs), ex.rank, ptr(g32), K, 0.0, ptr(cm), K)
            img = torch.empty((K, D), dtype=torch.float32, device=dev)
            zero = torch.zeros(D, dtype=torch.float32, device=dev)
            ex.expand(K, 1, panel_code(("denoised",)), None, 0, out=ptr(img), coeff=cm, ldc=K, mean=zero)
            ctx.sync()
            den_img = img.cpu().numpy().astype(np.float64)
        else:
            den_img = np.zeros((K, D), dtype=np.float64)
    ctx.sync()

    out = {}
    if not corr:
        sx = x64.sum(axis=1)[:, None]
        div = sx if stat == "mean" else 1.0
        raw = den = None
        if do_raw:
            raw = ((acc_raw.cpu().numpy() + centre32.astype(np.float64)[None, :] * sx) / div).astype(np.float32)
        if factor_sums:
            den = ((den_img + mean32[None, :] * sx) / div).astype(np.float32)
        if "raw" in kinds:
            out["raw"] = raw
        if "denoised" in kinds:
            out["denoised"] = den
        if "residual" in kinds:
            out["residual"] = raw - den
        return out
    xf = x32.astype(np.float64)
    sx, sxx = xf.sum(axis=1), (xf * xf).sum(axis=1)
    if do_raw:
        m = mom_raw.cpu().numpy()
        out["raw"] = _pearson(acc_raw.cpu().numpy(), m[:D], m[D:], sx, sxx, T)
    if P:
        a = split_panels(acc_ex.cpu().numpy(), d1, P, d2)
        m = split_panels(mom_ex.cpu().numpy().reshape(2, P * D), d1, P, d2)
        for j, k in enumerate(panels):
            out[k] = _pearson(a[j], m[j][0], m[j][1], sx, sxx, T)
    return out


def _pearson(sxz, sz, szz, sx, sxx, T):
    """r = (S xz - S x S z / T) / sqrt((S xx - (S x)^2 / T) (S zz - (S z)^2 / T)) in float64 from the float64 sums; 0
    where a variance is <= 0; clipped to [-1, 1] and rounded once to float32.  The block sums behind S z and S zz are
    fp32 chains: S zz is known to GAMMA S zz and (S z)^2 / T to 2 GAMMA S zz, so a pixel variance of at most
    3 GAMMA S zz cannot be told from that of a constant pixel and counts as 0."""
    num = sxz - sx[:, None] * sz[None, :] / T
    vx = sxx - sx * sx / T
    vz = szz - sz * sz / T
    den = vx[:, None] * vz[None, :]
    ok = (vx[:, None] > 0) & (vz[None, :] > 3.0 * GAMMA * szz[None, :])
    r = np.where(ok, num / np.sqrt(np.where(ok, den, 1.0)), 0.0)
    return np.clip(r, -1.0, 1.0).astype(np.float32)
