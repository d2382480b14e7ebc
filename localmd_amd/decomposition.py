"""
localmd_decomposition / compute_lowrank_factorized_svd / projected_svd on MI355X.

Host side of the blockwise-PMD hot path: same call signature, defaults, printed phase
messages and error behaviour as /root/reference/localmd/decomposition.py:643-909, with every
numeric stage executed by libpmd_hip.so (include/pmd_hip.h) on the HIP device.  PyTorch is
used for device memory, streams and H2D/D2H copies only.  There is no CPU fallback.  The movie
sources the driver works on, resident (_Movie) or streamed (_StreamedMovie), are _movie.py's.

Additions to the reference signature (keyword-only): ``seed`` (counter-based device RNG seed;
default: one draw from np.random), ``device`` (HIP device index), ``thresholds`` (inject the
two roughness cut-offs instead of simulating them), ``sim_iters``, ``return_diagnostics``,
``orthogonalizer``: how the mixing matrix P with (UP)^T(UP) = I is built when R > frames --
"eigh" is the reference's eigendecomposition (decomposition.py:984-996); "cholesky" uses the
Cholesky factor of the same Gram matrix (P differs by an orthogonal factor that the final SVD
absorbs, so R, s, Vt are the same); "auto" (default) = cholesky with eigh as fallback.
``distributed=True`` (one process per GPU, torch.distributed initialised): every rank owns a band of tile
rows and keeps only the pixel slab those tiles touch (statistics, standardisation, tile fits and the movie
projection run on the slab); sums over pixels (background projection) and over component rows (the two
Gram matrices of the Cholesky route) are all-reduced, per-tile results are gathered, R is collected on rank 0.
Rank 0 returns the PMDArray; on the row-sharded route the other ranks return None.  Random draws (seed,
frame sample, frame windows) are rank 0's.
``stream``: True reads the movie from its host source in ``frame_batch_size`` batches (rounded down to whole
1024-frame chunks) instead of holding it in HBM - pass 1 computes the statistics and gathers the fit frames and the
background sample, pass 2 projects every batch on the spatial basis (pmd_loader.py:203-291, :316-346); uint16 / int16
sources travel in their own dtype.  False: the resident path.  None (default): streams only when the resident plan's
raw + standardised movie copies do not fit in the free device memory.  Single GPU, host sources only.
"""
import datetime
import functools
import math
import sys
import os
import time
from typing import Callable, NamedTuple, Optional

import numpy as np
import scipy.sparse
from scipy.sparse import coo_matrix

from . import grid
from ._lib import Context, ptr, PMDLibraryError, c_i, C
from ._movie import (_Movie, _StreamedMovie, _device_free_bytes, _f32, _i32, _plan_mode, _round_up, _side_stream,
                     _stream_source_problem, _torch)
# the planning helpers of the streamed mode stay reachable under the names they had in this module
from ._movie import (_gather_maps, _stream_batch_frames, _stream_batches, _stream_dtype, _stream_fit_bytes,  # noqa: F401
                     _usable_free_bytes)
from .pmdarray import PMDArray
from .parallel import Dist, ownership_plan, tile_partition

STREAM_PRUNE = 5
QUIET = False
# Cholesky route, kept null direction: the rotated-in constant vector is carried next to the joint SVD only when its pivot is
# below this fraction of the mean diagonal of C (pure rounding: 1e-10 ... 1e-8 measured); a resolved direction goes through
# the joint SVD like any other.
NULL_PIVOT_REL = 1e-6


def display(msg):
    """Timestamped, flushed phase message (decomposition.py:28-34)."""
    if QUIET:
        return
    tag = "[" + datetime.datetime.today().strftime("%y-%m-%d %H:%M:%S") + "]: "
    sys.stdout.write(tag + msg + "\n")
    sys.stdout.flush()


def _dbg(name, t):
    """PMD_DEBUG=1: synchronise and report range / finiteness of an intermediate tensor."""
    if not os.environ.get("PMD_DEBUG"):
        return
    torch = _torch()
    torch.cuda.synchronize()
    tf = t.float() if t.dtype != torch.float64 else t
    finite = bool(torch.isfinite(tf).all())
    print(f"[pmd-debug] {name}: shape={tuple(t.shape)} finite={finite} absmax={float(tf.abs().max()):.4g}", flush=True)


def _stream_tile_bytes(n_tiles, rpad, dpad, ld_fit, ld_proj, tile_batch_bytes):
    """Device bytes of the tile stage and of the projection blocks of pass 2: the per-tile bases U and U W (kept for
    every tile) plus the per-tile traces and kernel temporaries - the per_tile_bytes estimate of the driver, which are
    held for all tiles at once or, above tile_batch_bytes, for one batch of tiles at a time."""
    per_tile = 3 * rpad * max(ld_fit, ld_proj) * 4 + 8 * rpad * dpad * 4 + (6 * rpad * rpad * 8 if rpad > 64 else 0)
    return n_tiles * 2 * rpad * dpad * 4 + min(n_tiles * per_tile, max(int(tile_batch_bytes), 8 * per_tile))


def _to_host(t):
    """Device tensor -> NumPy through page-locked memory (PCIe rate instead of pageable-copy rate).
    The array owns its pinned block until it is garbage collected."""
    torch = _torch()
    out = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    out.copy_(t, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return out.numpy()


def _sparse_u(ut_host, ranks, pix_f, block_weights, inv_cumw_rows, n_rows):
    """Sparse assembly of decomposition.py:812-853 (COO triplets, weights, row normalisation),
    vectorised.  ut_host: (n_tiles, 64, dpad) float32; pix_f: (n_tiles, d) row ids of the output
    matrix.  Values are float64: (float64(U) * w) * (1/cumw), like the reference."""
    n_tiles, _, _ = ut_host.shape
    d = pix_f.shape[1]
    offsets = np.concatenate([[0], np.cumsum(ranks)]).astype(np.int64)
    total = int(offsets[-1])
    w_flat = block_weights.reshape(-1, order="F").astype(np.float64)
    rows_l, cols_l, vals_l = [], [], []
    for rk in np.unique(ranks):
        if rk == 0:
            continue
        sel = np.nonzero(ranks == rk)[0]
        u = ut_host[sel, :rk, :d].astype(np.float64)            # (m, rk, d)
        vals = u * w_flat[None, None, :]
        rows = np.broadcast_to(pix_f[sel][:, None, :], vals.shape)
        vals = vals * inv_cumw_rows[rows]
        cols = offsets[sel][:, None, None] + np.arange(rk)[None, :, None]
        cols = np.broadcast_to(cols, vals.shape)
        rows_l.append(rows.reshape(-1))
        cols_l.append(cols.reshape(-1))
        vals_l.append(vals.reshape(-1))
    if vals_l:
        rows = np.concatenate(rows_l)
        cols = np.concatenate(cols_l)
        vals = np.concatenate(vals_l)
        keep = vals != 0  # the reference's dia.dot(coo) drops exact zeros
        u_r = coo_matrix((vals[keep], (rows[keep], cols[keep])), shape=(n_rows, total))
    else:
        u_r = coo_matrix((n_rows, total), dtype=np.float64)
    return u_r, offsets


def _virtual_ranks(ranks_dev, nvt):
    """ranks of the blocks of 64 component rows of every tile: tile t with rank k -> min(max(k - 64 h, 0), 64), h < nvt."""
    torch = _torch()
    if nvt == 1:
        return ranks_dev
    h = 64 * torch.arange(nvt, device=ranks_dev.device, dtype=ranks_dev.dtype)
    return torch.clamp(ranks_dev[:, None] - h[None, :], 0, 64).reshape(-1).contiguous()


def _apply_hook(fn, arr):
    """arr: (n_tiles, ...) device view.  The reference calls the denoiser once per block (decomposition.py:300, :310);
    a callable with a true ``batched`` attribute receives all tiles at once instead."""
    torch = _torch()
    if getattr(fn, "batched", False):
        out = fn(arr.contiguous())
        if tuple(out.shape) != tuple(arr.shape):
            raise ValueError("denoiser returned shape {} for input {}".format(tuple(out.shape), tuple(arr.shape)))
        arr.copy_(torch.as_tensor(out, dtype=torch.float32, device=arr.device))
        return
    for i in range(arr.shape[0]):
        out = fn(arr[i].contiguous())
        if tuple(out.shape) != tuple(arr[i].shape):
            raise ValueError("denoiser returned shape {} for input {}".format(tuple(out.shape), tuple(arr[i].shape)))
        arr[i].copy_(torch.as_tensor(out, dtype=torch.float32, device=arr.device))


def _tiles_decompose(ctx, args, ws, hook_geom, temporal_denoiser, spatial_denoiser):
    """pmd_tiles_decompose, or its three resumable parts around the denoiser hooks of single_block_md
    (decomposition.py:300 temporal_denoiser on V_ds (r, t); :304-313 spatial_denoiser on S as (r, b1, b2)).
    The hooks get float32 device tensors (torch) and must return tensors of the same shape."""
    torch = _torch()
    if temporal_denoiser is None and spatial_denoiser is None:
        ctx.call("pmd_tiles_decompose", *args, ptr(ws), ws.numel())
        return
    n, b1, b2, P_pool, r, a_f, t_crop, ldv, n_rows, dpad = hook_geom
    rp = ctx.lib.pmd_tile_rpad(r)
    off_v, off_s = C.c_size_t(0), C.c_size_t(0)
    rc = ctx.lib.pmd_tiles_hook_offsets(n, b1, b2, P_pool, r, a_f, t_crop, ldv, n_rows, C.byref(off_v), C.byref(off_s))
    if rc != 0:
        raise ValueError("pmd_tiles_hook_offsets failed ({})".format(rc))
    flat = ws.view(torch.uint8).reshape(-1)
    r = min(r, t_crop // a_f, P_pool, r + 10)   # the components that exist (pmd_tiles_decompose: bins / pooled pixels may be fewer)
    vds = flat[off_v.value:off_v.value + n * rp * ldv * 4].view(torch.float32).view(n, rp, ldv)[:, :r, :t_crop]
    s_arr = flat[off_s.value:off_s.value + n * rp * dpad * 4].view(torch.float32).view(n, rp, dpad)[:, :r, :b1 * b2]
    ctx.call("pmd_tiles_decompose_staged", *args, ptr(ws), ws.numel(), 1)
    if temporal_denoiser is not None:
        _apply_hook(temporal_denoiser, vds)
    ctx.call("pmd_tiles_decompose_staged", *args, ptr(ws), ws.numel(), 2)
    if spatial_denoiser is not None:
        # tile pixel q = il + b1 * jl  ->  (r, b1, b2) as the reference's F-order reshape + transpose(2, 0, 1)
        _apply_hook(spatial_denoiser, s_arr.view(n, r, b2, b1).transpose(2, 3))
    ctx.call("pmd_tiles_decompose_staged", *args, ptr(ws), ws.numel(), 4)


def _orthogonalize(ctx, G, R, M, m, ldm):
    """Device A15.  Returns (P tensor (R, ldp), R')."""
    torch = _torch()
    mm = m if M is not None else R
    ldp = mm
    P = torch.empty((R, ldp), dtype=torch.float32, device=ctx.device)
    ws_bytes = ctx.lib.pmd_orthogonalize_workspace_bytes(R, mm, 1 if M is not None else 0)
    ws = ctx.workspace(ws_bytes)
    rp = c_i(0)
    ctx.call("pmd_orthogonalize", ptr(G), R, ptr(M), mm, ldm, ptr(P), ldp, C.byref(rp), ptr(ws), ws.numel())
    return P, int(rp.value)


def _projected_svd_dev(ctx, P, rows_p, ldp, V, n1, n2, ldv):
    torch = _torch()
    nk = min(n1, n2)
    R_out = torch.empty((rows_p, nk), dtype=torch.float32, device=ctx.device)
    s_out = torch.empty((nk,), dtype=torch.float32, device=ctx.device)
    Vt_out = torch.empty((nk, n2), dtype=torch.float32, device=ctx.device)
    ws_bytes = ctx.lib.pmd_projected_svd_workspace_bytes(rows_p, n1, n2)
    ws = ctx.workspace(ws_bytes)
    ctx.call("pmd_projected_svd", ptr(P), rows_p, ldp, ptr(V), n1, n2, ldv, ptr(R_out), nk, ptr(s_out), ptr(Vt_out), n2,
             ptr(ws), ws.numel())
    return R_out, s_out, Vt_out


def projected_svd(projection, data, device=None):
    """(projection @ left, s, right) for the SVD of ``data`` via its Gram matrix
    (decomposition.py:1013-1060).  Host arrays in, host arrays out; computed on the device."""
    torch = _torch()
    ctx = Context(0 if device is None else device)
    try:
        d1, d2 = data.shape
        if d1 <= d2:
            display("Short matrix, using leftward SVD routine")
        else:
            display("Tall matrix, using rightward SVD routine")
        P = _f32(ctx, np.asarray(projection))
        V = _f32(ctx, np.asarray(data))
        R_out, s_out, Vt_out = _projected_svd_dev(ctx, P, P.shape[0], P.shape[1], V, d1, d2, d2)
        ctx.sync()
        return R_out.cpu().numpy(), s_out.cpu().numpy(), Vt_out.cpu().numpy()
    finally:
        ctx.close()


def compute_lowrank_factorized_svd(u: coo_matrix, v: np.ndarray, only_left: bool = False, device=None):
    """Orthonormalising mixing matrix of the factorisation u @ v (decomposition.py:936-1010).
    ``u`` is a general scipy sparse matrix here, so U^T U is formed with scipy (as the reference
    does, :974) and uploaded; the eigendecomposition and all dense products run on the device."""
    torch = _torch()
    ctx = Context(0 if device is None else device)
    try:
        u = scipy.sparse.csr_matrix(u)
        R = u.shape[1]
        G = _f32(ctx, np.asarray((u.T.dot(u)).todense()))
        v32 = np.ascontiguousarray(v, dtype=np.float32)
        M = _f32(ctx, v32) if R > v.shape[1] else None
        P, rp = _orthogonalize(ctx, G, R, M, v.shape[1], v.shape[1])
        P = P[:, :rp].contiguous()
        if only_left:
            ctx.sync()
            return P.cpu().numpy()
        utuv = _f32(ctx, np.asarray(u.T.dot(u).dot(v)))
        nt = torch.empty((rp, v.shape[1]), dtype=torch.float32, device=ctx.device)
        ctx.call("pmd_gemm", 1, 0, rp, v.shape[1], R, 1.0, ptr(P), rp, ptr(utuv), v.shape[1], 0.0, ptr(nt), v.shape[1])
        R_out, s_out, Vt_out = _projected_svd_dev(ctx, P, R, rp, nt, rp, v.shape[1], v.shape[1])
        ctx.sync()
        return R_out.cpu().numpy(), s_out.cpu().numpy(), Vt_out.cpu().numpy()
    finally:
        ctx.close()


# ---- the driver: localmd_decomposition and its stages ("driver stages").  A stage is a module-level
# function (or a small class) with explicit inputs and outputs; the tensors a stage hands on are exactly the ones
# that must stay alive, everything else dies with the stage's frame.


class _Laps:
    """Phase timer of one call.  lap() synchronises only when diagnostics were asked for (return_diagnostics=True),
    so a plain call keeps the host running ahead of the device."""

    def __init__(self, ctx, synchronise):
        self.ctx, self.synchronise, self.timings = ctx, synchronise, {}

    def __call__(self, name, t0):
        if self.synchronise:
            self.ctx.sync()
        self.timings[name] = self.timings.get(name, 0.0) + time.perf_counter() - t0


class _PixelStats(NamedTuple):
    mean_dev: object      # (resident pixels,) per-pixel mean ...
    std_dev: object       # ... and noise level
    basis_dev: object     # (D, K) spatial background basis of the whole field of view, or None (K <= 0)


class _Geom(NamedTuple):
    """Tile grid of one call (host integers and the pyramid weights)."""
    d1: int
    d2: int
    D: int
    order: str
    b1: int
    b2: int
    d: int                # pixels of a tile
    block_sizes: list
    block_weights: object
    o1: list              # tile origins along the two axes
    o2: list


class _TileTables(NamedTuple):
    """Pixel lists and pooling maps of the tile kernels."""
    pix_c: object         # (n_tiles, d) C-order pixel ids, host
    origins: object
    pix_dev: object
    pool_q_dev: object
    pool_idx_dev: object
    pool_w_dev: object
    pool_cols: int
    P_pool: int
    dpad: int
    n_tiles: int


class _Standardized(NamedTuple):
    xf: object            # standardised, background-filtered fit frames, pixel-major (rows_alloc x ld_f)
    xs_full: object       # standardised whole movie (rows_alloc x ld_T); None: single-copy plan or streamed
    pj_dev: object        # (K, ld_f) background traces B^T X of the fit frames, or None
    ld_f: int
    ld_T: int
    single_copy: bool     # as decided (the request holds only where the plan applies)
    all_frames: bool


class _Tiles(NamedTuple):
    """Result of the tile stage.  After _virtual_tiles a "tile" is a block of 64 component rows."""
    ut_dev: object        # (n_tiles, rpad, dpad) spatial components
    stats_dev: object
    good_dev: object
    keep_dev: object
    ranks_dev: object
    lam_dev: object
    v_dev: object         # (n_tiles, rpad, ldv) traces of the fit frames - or, fitted in batches ...
    v_pieces: list        # ... the compacted traces of every batch (emptied once copied into v_cropped)
    ldv: int
    rpad: int
    nvt: int              # blocks of 64 component rows per tile
    r: int                # max_components in force
    n_tiles: int
    t_lo: int             # this rank's run of tiles
    t_hi: int
    runs: list
    batches: list         # [lo, hi) runs of local tiles fitted / projected together
    pix_c: object
    origins: object
    pix_dev: object
    pix_loc_dev: object   # pixel lists of this rank's tiles relative to its slab
    pairs: object         # overlapping tile pairs
    cumw: object          # summed pyramid weights per pixel
    cover: tuple          # cover tables of the CSR assembly
    thresholds: tuple
    sim_stats: object

    @property
    def n_loc(self):
        return self.t_hi - self.t_lo

    @property
    def batched(self):
        return len(self.batches) > 1


class _Columns(NamedTuple):
    """Column layout of U = [tile components | background]."""
    ranks: object         # (n_tiles,) host
    offsets: object       # first column of every tile, and the total
    col_off_dev: object
    w_dev: object         # pyramid weights of a tile's pixels
    Rt: int               # tile columns
    R: int                # with the background columns (one empty placeholder column when K <= 0, pmd_loader.py:301-302)
    Rc: int               # columns with content


def _check_options(dataset_obj, dtype, spatial_denoiser, temporal_denoiser, order, orthogonalizer, null_directions, stream,
                   distributed):
    if np.dtype(dtype) != np.float32:
        raise ValueError("only dtype='float32' is supported (the reference computes in float32 throughout)")
    for hook in (spatial_denoiser, temporal_denoiser):
        if hook is not None and not callable(hook):
            raise TypeError("spatial_denoiser / temporal_denoiser must be callables on torch device tensors")
    if order not in ("F", "C"):
        raise ValueError("order must be 'F' or 'C'")
    if orthogonalizer not in ("auto", "eigh", "cholesky"):
        raise ValueError("orthogonalizer must be 'auto', 'eigh' or 'cholesky'")
    if null_directions not in ("keep", "drop"):
        raise ValueError("null_directions must be 'keep' (the reference's rule) or 'drop'")
    if stream:
        problem = _stream_source_problem(dataset_obj, distributed)
        if problem is not None:
            raise ValueError(problem)


def _stream_fit_tile_bytes(lib, movie, n_fit, block_sizes, max_components, temporal_avg_factor, tile_batch_bytes):
    """_stream_tile_bytes for the tile grid of `block_sizes` fitted on n_fit frames."""
    blocks = grid.update_block_sizes(list(block_sizes), (movie.d1, movie.d2), display=None)
    o1, o2 = grid.tile_origins((movie.d1, movie.d2), blocks)
    r_fit = max(1, min(int(max_components), n_fit // int(temporal_avg_factor)))
    d = int(blocks[0]) * int(blocks[1])
    return _stream_tile_bytes(len(o1) * len(o2), int(lib.pmd_tile_rpad(r_fit)), max(int(lib.pmd_tile_dpad(d)), d),
                              int(lib.pmd_time_ld(n_fit)), int(lib.pmd_time_ld(movie.project_frames)), tile_batch_bytes)


def _draw_sample(T, dist):
    """The (<= 1000) frames the background basis is estimated from: one np.random draw, rank 0's."""
    return dist.broadcast_object(np.random.choice(list(range(T)), replace=False, size=min(1000, T)).tolist())


def _load_statistics_background(ctx, dist, own, dataset_obj, streamed, fit_request, K, seed, compute_normalizer, load_options,
                                lap):
    """PMDLoader.__init__ (pmd_loader.py:112-173): movie to HBM, statistics, background basis - and the frames to fit on.
    Streamed (the movie stays at its source and is read twice): pass 1 here, pass 2 in _ZBuilder.
    fit_request = (frame_range, window_chunks, max_components, temporal_avg_factor, block_sizes);
    load_options = (frame_batch_size, num_workers, tile_batch_bytes).
    Returns (movie, _PixelStats, frames, frame_range, window_chunks)."""
    torch = _torch()
    lib = ctx.lib
    frame_range, window_chunks, max_components, temporal_avg_factor, block_sizes = fit_request
    frame_batch_size, num_workers, tile_batch_bytes = load_options
    t0 = time.perf_counter()
    if streamed:
        movie = _StreamedMovie(ctx, dataset_obj, frame_batch_size, num_workers=num_workers)
    else:
        movie = _Movie(ctx, dataset_obj, frame_batch_size, rows=(own.i_lo, own.i_hi) if dist.enabled else None,
                       num_workers=num_workers)
    T, D, Dl = movie.T, movie.d1 * movie.d2, movie.D    # Dl: resident pixels (= D unless distributed)
    lap("upload", t0)
    display("Computing Video Statistics")
    if compute_normalizer:
        display("We are normalizing each pixel by a noise variance estimate")
    else:
        display("We are not normalizing each pixel by a noise variance estimate")
    display("Calculating mean and noise variance")
    t0 = time.perf_counter()
    mean_dev = torch.empty(Dl, dtype=torch.float32, device=ctx.device)
    std_dev = torch.empty(Dl, dtype=torch.float32, device=ctx.device)
    sample = frames = None
    if streamed:
        # Order of the np.random draws (behaviour): background sample, then the fit windows - the resident path's
        # order, made BEFORE pass 1, which gathers those frames: a seeded call fits the same frames in both modes.
        sample = _draw_sample(T, dist) if K > 0 else None
        frames, frame_range, window_chunks = grid.select_frames(T, frame_range, window_chunks, display, dist.broadcast_object)
        movie.check_fit_frames(len(frames), len(sample or []), _stream_fit_tile_bytes(
            lib, movie, len(frames), block_sizes, max_components, temporal_avg_factor, tile_batch_bytes))
    movie.statistics(compute_normalizer, mean_dev, std_dev, frames, sample)
    display("Finished mean and noise variance")
    lap(movie.statistics_phase, t0)

    t0 = time.perf_counter()
    basis_dev = None
    if K > 0:
        if sample is None:
            sample = _draw_sample(T, dist)    # resident: drawn after the statistics (order of the np.random draws)
        xs_s, ld_s = movie.standardized("sample", mean_dev, std_dev, sample)
        if dist.enabled:
            # the (<= 1000 frame) sample is small: every rank contributes its owned pixels, all get the whole
            # sample and compute the same basis (same counter-based test matrix)
            xs_all = torch.zeros((_round_up(D, 1024) + 1024, ld_s), dtype=torch.float32, device=ctx.device)
            xs_all[own.O_lo:own.O_hi] = xs_s[own.O_lo - own.P_lo:own.O_hi - own.P_lo]
            dist.gather_runs(xs_all, own.owned)
            xs_s = xs_all
        basis_dev = torch.empty((D, K), dtype=torch.float32, device=ctx.device)
        ws = ctx.workspace(lib.pmd_background_rsvd_workspace_bytes(D, len(sample), K))
        ctx.call("pmd_background_rsvd", ptr(xs_s), D, len(sample), ld_s, K, seed, ptr(basis_dev), ptr(ws), ws.numel())
        del xs_s
    lap("background", t0)
    if frames is None:
        # resident: the fit windows are drawn (and announced) after the background sample
        frames, frame_range, window_chunks = grid.select_frames(T, frame_range, window_chunks, display, dist.broadcast_object)
    return movie, _PixelStats(mean_dev, std_dev, basis_dev), frames, frame_range, window_chunks


def _geometry(fov, block_sizes, order):
    block_sizes = grid.update_block_sizes(block_sizes, fov, display=display)
    b1, b2 = block_sizes
    o1, o2 = grid.tile_origins(fov, block_sizes)
    return _Geom(fov[0], fov[1], fov[0] * fov[1], order, b1, b2, b1 * b2, block_sizes,
                 grid.block_weight_matrix(block_sizes, dtype=np.float32), o1, o2)


class _ThresholdSim:
    """The two roughness cut-offs (decomposition.py:700-711).  The simulation depends on nothing but the block shape: it
    is enqueued on the second stream at construction, next to the HBM-bound standardise / filter passes, and joined by
    result(), which the tile stage calls right before its first launch.  Injected thresholds are handed through."""

    def __init__(self, ctx, geom, window_chunks, sim_iters, sim_conf, seed, thresholds):
        torch = _torch()
        self.sim_conf, self.thresholds, self.side, self.sim_dev = sim_conf, None, None, None
        if thresholds is not None:
            spatial_threshold, temporal_threshold = thresholds
            self.thresholds = (spatial_threshold, temporal_threshold)
            return
        sc = ctx.side()
        with torch.cuda.stream(sc.stream):
            ws_sim = sc.workspace(ctx.lib.pmd_threshold_sim_workspace_bytes(geom.b1, geom.b2, int(window_chunks), int(sim_iters)))
            self.sim_dev = torch.empty((sim_iters, 2), dtype=torch.float32, device=ctx.device)
            sc.call("pmd_threshold_sim", geom.b1, geom.b2, int(window_chunks), int(sim_iters), seed, ptr(self.sim_dev),
                    ptr(ws_sim), ws_sim.numel())
        self.side = sc

    def result(self):
        """(spatial threshold, temporal threshold, simulated statistics or None)."""
        if self.thresholds is not None:
            spatial_threshold, temporal_threshold = self.thresholds
            return spatial_threshold, temporal_threshold, None
        self.side.sync()
        sim_stats = self.sim_dev.cpu().numpy()
        self.sim_dev = None
        return np.percentile(sim_stats[:, 0], self.sim_conf), np.percentile(sim_stats[:, 1], self.sim_conf), sim_stats


def _standardize_filter(ctx, dist, own, movie, stats, frames, K, single_copy, pixel_weighting, temporal_avg_factor, lap):
    """Standardise, background-filter, transpose (pmd_loader.py:348-389).

    Memory plan for movies that fill the HBM (BASELINE configs 4 / 5: 84 GB): with every frame fitted the filtered
    copy X_f = X - B (B^T X) replaces the standardised one in place, and the movie projection of the last stage is
    formed as (UW)^T X = (UW)^T X_f + ((UW)^T B) (B^T X) - the second term is a rank-K product of quantities the
    global stage holds anyway (the background strip of U^T U, the background traces).  One movie-sized array
    instead of two (three with the raw copy).  `single_copy=None`: automatic, above 1/8 of the device memory."""
    torch = _torch()
    lib = ctx.lib
    T, Dl, Tf = movie.T, movie.D, len(frames)
    mean_dev, std_dev, basis_dev = stats
    t0 = time.perf_counter()
    all_frames = frames == list(range(T))
    xs_full, ld_T = movie.standardized("all", mean_dev, std_dev)    # streamed: no such copy, Z is formed from pass 2
    if all_frames and xs_full is not None:
        xs_init, ld_f = xs_full, ld_T
    else:
        xs_init, ld_f = movie.standardized("fit", mean_dev, std_dev, frames)
    pj_dev = None
    movie.release()      # lifetime: the standardised copies are written, the raw frames are not read again
    if single_copy is None:
        single_copy = 4.0 * Dl * T > torch.cuda.get_device_properties(ctx.device).total_memory / 8.0
    # streamed: nothing but the filter reads the standardised fit frames (Z comes from pass 2), so it filters in place
    sole_reader = movie.streamed
    single_copy = (bool(single_copy) and all_frames and K > 0 and pixel_weighting is None
                   and Tf % int(temporal_avg_factor) == 0 and not sole_reader)
    in_place = single_copy or sole_reader
    if K > 0:
        pj_dev = torch.zeros((K, ld_f), dtype=torch.float32, device=ctx.device)
        # projection on the background basis: a sum over pixels - owned pixels here, summed over the ranks
        ws = ctx.workspace(lib.pmd_bg_project_workspace_bytes(own.O_hi - own.O_lo, Tf))
        ctx.call("pmd_bg_project", ptr(xs_init[own.O_lo - own.P_lo:]), own.O_hi - own.O_lo, Tf, ld_f, ptr(basis_dev[own.O_lo:]), K,
                 ptr(pj_dev), ld_f, ptr(ws), ws.numel())
        dist.all_reduce(pj_dev)
        if in_place:
            xf = xs_init                     # filtered in place (the kernel is element-wise)
            xs_full = None                   # lifetime: the single copy is xf from here on
        else:
            xf = torch.empty_like(xs_init)   # bg_filter writes all ld columns of the resident pixel rows
            if xf.shape[0] > Dl:
                xf[Dl:].zero_()
        ctx.call("pmd_bg_filter", ptr(xs_init), ptr(xf), Dl, Tf, ld_f, ptr(basis_dev[own.P_lo:]), K, ptr(pj_dev), ld_f)
    else:
        xf = xs_init.clone() if (pixel_weighting is not None and not in_place) else xs_init
    if in_place:
        xs_init = None       # lifetime: xf is the only reference to the (filtered) copy
    if pixel_weighting is not None:
        pw = _f32(ctx, np.asarray(pixel_weighting, dtype=np.float32).reshape(-1)[own.P_lo:own.P_hi])
        ctx.call("pmd_scale_rows", ptr(xf), Dl, Tf, ld_f, ptr(pw))
    lap("standardize_filter", t0)
    crop = (Tf // temporal_avg_factor) * temporal_avg_factor
    if crop < Tf:
        # The tile fits use the first `crop` fitted frames only (decomposition.py:773-774, :796), and the tile
        # kernels walk the time axis in 32-frame chunks relying on zeros behind the last frame they are given:
        # frames crop .. Tf - 1 of the filtered copy must not leak into the contractions.  (Found by the seeded
        # fuzz of round 2: every draw with frames % temporal_avg_factor != 0 was off by ~1e-3 in its tile bases.)
        if xs_init is not None and xf.data_ptr() == xs_init.data_ptr():
            xf = xs_init.clone()    # xs_init may be the standardised movie the V projection still needs
        xf[:, crop:Tf].zero_()
    return _Standardized(xf, xs_full, pj_dev, ld_f, ld_T, single_copy, all_frames)


def _tile_tables(ctx, geom, spatial_avg_factor):
    """Tile grid (decomposition.py:721-773): pixel lists and pooling maps, on the host and uploaded."""
    lib = ctx.lib
    pix_c, origins = grid.tile_pixel_lists((geom.d1, geom.d2), geom.block_sizes, geom.o1, geom.o2)
    pool_q, pool_idx, pool_w, _ = grid.pooling_maps(geom.block_sizes, int(spatial_avg_factor))
    P_pool = pool_q.shape[0]
    dpad = lib.pmd_tile_dpad(geom.d)
    if dpad < 0 or lib.pmd_tile_dpad(P_pool) < 0:
        raise ValueError("block of {} x {} pixels is larger than the supported maximum (65536 pixels)".format(geom.b1, geom.b2))
    pix_dev = _i32(ctx, pix_c)
    return _TileTables(pix_c, origins, pix_dev, _i32(ctx, pool_q), _i32(ctx, pool_idx), _f32(ctx, pool_w), pool_q.shape[1],
                       P_pool, dpad, pix_c.shape[0])


class _TileFit(NamedTuple):
    """What every tile fit is told (the arguments of single_block_md, decomposition.py:237-320)."""
    r: int
    a_f: int
    thr_s32: float
    thr_t32: float
    max_fail: int
    seed: int
    temporal_denoiser: object
    spatial_denoiser: object


def _fit_tiles(ctx, geom, tabs, fit, arrays, x, ld, n_rows, n_frames, pix, n, g0, v_out, ldv, n_win=1):
    """pmd_tiles_decompose (with the denoiser hooks, if any) of the n tiles from global index g0 on n_frames frames of x:
    the one place that lays out its arguments, sizes its workspace and describes it to the hooks.  x may be only the
    band of n_rows pixel rows the tiles touch, with pixel lists `pix` relative to it.  The Gaussian matrix of
    (tile, window) is logical array tile * n_win + window; the results go to rows g0.. of `arrays`, the traces to v_out."""
    ut_dev, stats_dev, good_dev, keep_dev, ranks_dev, lam_dev = arrays
    b1, b2, P_pool = geom.b1, geom.b2, tabs.P_pool
    # workspace: requested immediately before the call that uses it (the next larger request replaces the buffer)
    ws = ctx.workspace(ctx.lib.pmd_tiles_workspace_bytes(n, b1, b2, P_pool, fit.r, fit.a_f, n_frames, ldv, n_rows))
    args = (ptr(x), ld, n_rows, n_frames, ptr(pix), n, b1, b2, ptr(tabs.pool_q_dev), tabs.pool_cols, P_pool,
            ptr(tabs.pool_idx_dev), ptr(tabs.pool_w_dev), fit.r, fit.a_f, fit.thr_s32, fit.thr_t32, fit.max_fail, fit.seed,
            g0 * n_win, n_win, ptr(ut_dev[g0:]), ptr(v_out), ldv, ptr(stats_dev[g0:]), ptr(good_dev[g0:]), ptr(keep_dev[g0:]),
            ptr(ranks_dev[g0:]), ptr(lam_dev[g0:]))
    _tiles_decompose(ctx, args, ws, (n, b1, b2, P_pool, fit.r, fit.a_f, n_frames, ldv, n_rows, tabs.dpad),
                     fit.temporal_denoiser, fit.spatial_denoiser)


def _fit_tiles_in_batches(ctx, geom, tabs, fit, arrays, own, std, crop, batches, pix_loc_dev, rpad, nvt):
    """Tile fits above tile_batch_bytes: one batch of tiles at a time, its traces compacted to the kept components right
    away.  Returns the compacted pieces."""
    torch = _torch()
    ranks_dev = arrays[4]
    ldv, v_pieces = std.ld_f, []
    for b0, b1_ in batches:
        nb_, g0 = b1_ - b0, own.t_lo + b0
        vb = torch.empty((nb_, rpad, ldv), dtype=torch.float32, device=ctx.device)
        # the band of resident pixels the batch touches (tiles are in tile-row order): the temporal binning of the
        # sketch walks only these rows instead of the whole movie once per batch (409 ms of 1.46 s at config 5)
        lo_pix = int(tabs.pix_c[g0:g0 + nb_].min()) - own.P_lo
        n_band = int(tabs.pix_c[g0:g0 + nb_].max()) + 1 - own.P_lo - lo_pix
        pix_b = (pix_loc_dev[b0:b1_] - lo_pix).contiguous()
        _fit_tiles(ctx, geom, tabs, fit, arrays, std.xf[lo_pix:], std.ld_f, n_band, crop, pix_b, nb_, g0, vb, ldv)
        rk = _virtual_ranks(ranks_dev[g0:g0 + nb_], nvt)     # blocks of 64 component rows
        off_b = (torch.cumsum(rk, 0) - rk).to(torch.int32)
        rows_b = int(rk.sum().item())
        piece = torch.zeros((max(rows_b, 1), crop), dtype=torch.float32, device=ctx.device)
        ctx.call("pmd_compact_rows", ptr(vb), ldv, ptr(off_b), ptr(rk), crop, ptr(piece), crop, nb_ * nvt)
        v_pieces.append(piece[:rows_b])
        del vb               # lifetime: one batch of traces at a time
    ctx.release_workspace()     # lifetime: the batch workspace (GBs) is not needed again
    return v_pieces


def _fit_tiles_in_windows(ctx, geom, tabs, fit, arrays, own, std, win, pix_loc_dev, v_dev, rpad, nvt):
    """Several temporal windows: first window = single_block_md, later ones fit the residual (decomposition.py:471-515);
    then the traces over all fitted frames, U_b^T X (get_temporal_projector, decomposition.py:518-523), into v_dev."""
    torch = _torch()
    lib = ctx.lib
    ut_dev, ranks_dev = arrays[0], arrays[4]
    t_lo, n_loc, Dl = own.t_lo, own.t_hi - own.t_lo, own.P_hi - own.P_lo
    b1, b2, dpad, xf = geom.b1, geom.b2, tabs.dpad, std.xf
    win_len, n_win = win.win_len, len(win.win_starts)
    ld_w = lib.pmd_time_ld(win_len)
    xw = torch.zeros((xf.shape[0], ld_w), dtype=torch.float32, device=ctx.device)
    vw = torch.empty((n_loc, rpad, ld_w), dtype=torch.float32, device=ctx.device)
    st_w = torch.zeros((n_loc, rpad, 2), dtype=torch.float32, device=ctx.device)
    gd_w = torch.zeros((n_loc, rpad), dtype=torch.int32, device=ctx.device)
    kp_w = torch.zeros((n_loc, rpad), dtype=torch.int32, device=ctx.device)
    for widx, w0 in enumerate(win.win_starts):
        xw[:Dl, :win_len] = xf[:Dl, w0:w0 + win_len]
        if widx == 0:
            # the denoiser hooks act in single_block_md only, i.e. in the first window (decomposition.py:476-488)
            _fit_tiles(ctx, geom, tabs, fit, arrays, xw, ld_w, Dl, win_len, pix_loc_dev, n_loc, t_lo, vw, ld_w, n_win)
            ctx.call("pmd_tiles_truncate", ptr(ut_dev[t_lo:]), dpad, ptr(ranks_dev[t_lo:]), n_loc, rpad)
        else:
            ws = ctx.workspace(lib.pmd_tiles_residual_workspace_bytes(n_loc, b1, b2, fit.r, fit.a_f, win_len, Dl))
            ctx.call("pmd_tiles_residual", ptr(xw), ld_w, Dl, win_len, ptr(pix_loc_dev), n_loc, b1, b2, fit.r, fit.a_f,
                     fit.thr_s32, fit.thr_t32, fit.max_fail, fit.seed, t_lo * n_win + widx, n_win,
                     ptr(ut_dev[t_lo:]), ptr(ranks_dev[t_lo:]), ptr(st_w), ptr(gd_w), ptr(kp_w), ptr(ws), ws.numel())
    del xw, vw               # lifetime: the window copies go before the traces are projected
    # (blocks of 64 component rows: a tile with rpad = 64 nvt rows is nvt such blocks with the same pixels)
    pix_blocks = pix_loc_dev if nvt == 1 else pix_loc_dev.repeat_interleave(nvt, dim=0)
    ctx.call("pmd_tiles_project", ptr(xf), std.ld_f, win.crop, ptr(pix_blocks), n_loc * nvt, geom.d, ptr(ut_dev[t_lo:]), dpad,
             ptr(v_dev[t_lo:]), std.ld_f, 2)


def _tile_stage(ctx, dist, own, geom, tabs, std, win, sim, fit_options, tile_batch_bytes, lap):
    """Local SVD of every tile of this rank's run (decomposition.py:775-838), gathered on all ranks.
    fit_options = (max_consecutive_failures, seed, temporal_denoiser, spatial_denoiser)."""
    torch = _torch()
    lib = ctx.lib
    n_tiles, dpad = tabs.n_tiles, tabs.dpad
    # Component rows of the per-tile arrays: 64 while max_components + 10 <= 64 (the MFMA-tiled kernels), a larger multiple
    # of 64 beyond (generic-width kernels, csrc/wide.hip) - max_components is unbounded, as in the reference
    # (decomposition.py:643-665).  The global stage works on blocks of 64 component rows: an array with rpad = 64 nvt rows is
    # handed to it as nvt "virtual tiles" per tile, [n * nvt][64][x], the same memory (_virtual_tiles).
    rpad = int(lib.pmd_tile_rpad(win.max_components))
    nvt = rpad // 64
    t0 = time.perf_counter()
    ldv = std.ld_f
    ut_dev = torch.empty((n_tiles, rpad, dpad), dtype=torch.float32, device=ctx.device)
    stats_dev = torch.zeros((n_tiles, rpad, 2), dtype=torch.float32, device=ctx.device)
    good_dev = torch.zeros((n_tiles, rpad), dtype=torch.int32, device=ctx.device)
    keep_dev = torch.zeros((n_tiles, rpad), dtype=torch.int32, device=ctx.device)
    ranks_dev = torch.zeros((n_tiles,), dtype=torch.int32, device=ctx.device)
    lam_dev = torch.zeros((n_tiles, rpad), dtype=torch.float64, device=ctx.device)
    arrays = (ut_dev, stats_dev, good_dev, keep_dev, ranks_dev, lam_dev)
    assert own.runs[-1][1] == n_tiles
    t_lo, n_loc = own.t_lo, own.t_hi - own.t_lo
    # pixel lists of this rank's tiles relative to its slab (the kernels that read the movie copies)
    pix_loc_dev = _i32(ctx, tabs.pix_c[t_lo:own.t_hi] - own.P_lo) if dist.enabled else tabs.pix_dev
    # streams: the threshold simulation, enqueued on the side stream before the standardise / filter passes, is joined here
    spatial_threshold, temporal_threshold, sim_stats = sim.result()
    fit = _TileFit(win.max_components, win.a_f, float(np.float32(spatial_threshold)), float(np.float32(temporal_threshold)),
                   int(fit_options[0]), fit_options[1], fit_options[2], fit_options[3])
    # Tile batches.  The per-tile temporaries ([tile][64][frames] traces and the kernels' workspace, ~3 such arrays)
    # grow with tiles x frames: 84 GB each at BASELINE config 5 (65 025 tiles x 5 000 frames).  Above
    # `tile_batch_bytes` the tiles are fitted (and later projected) in batches whose traces are compacted to the
    # kept components right away; one batch (every workload up to config 3's size) is the single-launch path.
    per_tile_bytes = 3 * rpad * int(max(ldv, std.ld_T)) * 4 + 8 * rpad * dpad * 4 + (6 * rpad * rpad * 8 if nvt > 1 else 0)
    batches = grid.tile_batches(n_loc, len(win.win_starts), per_tile_bytes, tile_batch_bytes)
    batched = len(batches) > 1
    v_dev = None if batched else torch.empty((n_tiles, rpad, ldv), dtype=torch.float32, device=ctx.device)
    v_pieces = []
    if n_loc > 0 and len(win.win_starts) == 1 and not batched:
        _fit_tiles(ctx, geom, tabs, fit, arrays, std.xf, std.ld_f, own.P_hi - own.P_lo, win.crop, pix_loc_dev, n_loc, t_lo,
                   v_dev[t_lo:], ldv)
    elif n_loc > 0 and len(win.win_starts) == 1:
        v_pieces = _fit_tiles_in_batches(ctx, geom, tabs, fit, arrays, own, std, win.crop, batches, pix_loc_dev, rpad, nvt)
    elif n_loc > 0:
        _fit_tiles_in_windows(ctx, geom, tabs, fit, arrays, own, std, win, pix_loc_dev, v_dev, rpad, nvt)
    for tns in arrays:      # collectives: one gather per array, in this order, on every rank
        dist.gather_runs(tns, own.runs)
    # geometry-only host tables of the assembly and of U^T U, built while the tile kernels run
    cumw = grid.cumulative_weights((geom.d1, geom.d2), geom.block_sizes, tabs.origins, geom.block_weights)
    cover = grid.cover_tables((geom.d1, geom.d2), geom.block_sizes, geom.o1, geom.o2)
    pairs = grid.overlap_pairs(tabs.origins, geom.block_sizes)
    ctx.sync()
    lap("tiles", t0)
    _dbg("ut", ut_dev); _dbg("tile_lambda", lam_dev)
    return _Tiles(ut_dev, stats_dev, good_dev, keep_dev, ranks_dev, lam_dev, v_dev, v_pieces, ldv, rpad, nvt, fit.r, n_tiles,
                  t_lo, own.t_hi, own.runs, batches, tabs.pix_c, tabs.origins, tabs.pix_dev, pix_loc_dev, pairs, cumw, cover,
                  (spatial_threshold, temporal_threshold), sim_stats)


class _PendingU:
    """The sparse U on its way to the host: the CSR arrays travel on the side stream while the global stage runs, and
    finish() joins the copy and builds the scipy matrix.  The handle keeps the device arrays alive until then."""

    def __init__(self, ctx, shape, nnz=0, device_arrays=None, u_r=None):
        torch = _torch()
        self.ctx, self.shape, self.u_r = ctx, shape, u_r      # u_r: already built on the host (nothing pending)
        self.device_arrays = device_arrays
        if device_arrays is None:
            return
        data_dev, idx_dev, indptr_dev = device_arrays
        side = _side_stream(ctx.device)
        self.host = (torch.empty(nnz, dtype=torch.float64, pin_memory=True),
                     torch.empty(nnz, dtype=torch.int32, pin_memory=True),
                     torch.empty(shape[0] + 1, dtype=torch.int64, pin_memory=True))
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(ctx.device))
        side.wait_event(ev)         # streams: the copy starts behind the CSR fill on the main stream
        with torch.cuda.stream(side):
            self.host[0].copy_(data_dev[:nnz], non_blocking=True)
            self.host[1].copy_(idx_dev[:nnz], non_blocking=True)
            self.host[2].copy_(indptr_dev, non_blocking=True)

    def finish(self):
        if self.device_arrays is not None:
            _side_stream(self.ctx.device).synchronize()
            data, idx, indptr = self.host
            self.u_r = scipy.sparse.csr_matrix((data.numpy(), idx.numpy(), indptr.numpy().astype(np.int32)), shape=self.shape)
            self.device_arrays = self.host = None
        return self.u_r


def _assemble_u(ctx, geom, tl, basis_dev, K, lap):
    """Sparse assembly (decomposition.py:752-857): CSR arrays built on the device.  Returns (_PendingU, _Columns)."""
    torch = _torch()
    d1, d2, D, order = geom.d1, geom.d2, geom.D, geom.order
    t0 = time.perf_counter()
    ranks_dev, ut_dev = tl.ranks_dev, tl.ut_dev
    ranks = ranks_dev.cpu().numpy().astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(ranks)]).astype(np.int64)
    Rt = int(offsets[-1])
    R = Rt + (K if K > 0 else 1)  # K <= 0: one empty placeholder column (pmd_loader.py:301-302)
    col_off_dev = _i32(ctx, offsets[:-1])
    w_dev = _f32(ctx, geom.block_weights.reshape(-1, order="F"))
    inv_cumw_dev = torch.from_numpy(np.ascontiguousarray(1.0 / tl.cumw.reshape(-1))).to(ctx.device)
    cov1_dev, cov2_dev = _i32(ctx, tl.cover[0]), _i32(ctx, tl.cover[1])
    o1_dev, o2_dev = _i32(ctx, geom.o1), _i32(ctx, geom.o2)
    row_nnz = torch.empty(D, dtype=torch.int64, device=ctx.device)
    n2 = len(geom.o2)
    order_f = 1 if order == "F" else 0
    ctx.call("pmd_csr_count", d1, d2, order_f, ptr(cov1_dev), ptr(cov2_dev), n2, ptr(ranks_dev), max(K, 0), ptr(row_nnz))
    indptr_dev = torch.zeros(D + 1, dtype=torch.int64, device=ctx.device)
    indptr_dev[1:] = torch.cumsum(row_nnz, 0)
    nnz = int(indptr_dev[-1].item())
    data_dev = torch.empty(max(nnz, 1), dtype=torch.float64, device=ctx.device)
    idx_dev = torch.empty(max(nnz, 1), dtype=torch.int32, device=ctx.device)
    zero_dev = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    ctx.call("pmd_csr_fill", d1, d2, order_f, geom.b1, ptr(cov1_dev), ptr(cov2_dev), ptr(o1_dev), ptr(o2_dev), n2,
             ptr(ranks_dev), ptr(col_off_dev), ptr(ut_dev), tl.ut_dev.shape[2], ptr(w_dev), ptr(inv_cumw_dev), ptr(basis_dev),
             max(K, 0), Rt, ptr(indptr_dev), ptr(data_dev), ptr(idx_dev), ptr(zero_dev), tl.rpad)
    if int(zero_dev.item()) == 0 and nnz < 2 ** 31:
        pending = _PendingU(ctx, (D, R), nnz, (data_dev, idx_dev, indptr_dev))
    else:
        # exact zeros present (the reference drops them, decomposition.py:853): host construction
        fov_ids = np.arange(D).reshape((d1, d2), order=order)
        pix_f = fov_ids.reshape(-1)[tl.pix_c]
        inv_rows = np.zeros(D)
        inv_rows[fov_ids.reshape(-1)] = 1.0 / tl.cumw.reshape(-1)
        u_local, _ = _sparse_u(ut_dev.cpu().numpy(), ranks, pix_f, geom.block_weights, inv_rows, D)
        if K > 0:
            basis_rows = np.empty((D, K), dtype=np.float32)
            basis_rows[fov_ids.reshape(-1)] = basis_dev.cpu().numpy()
            pending = _PendingU(ctx, (D, R), u_r=scipy.sparse.hstack([u_local, coo_matrix(basis_rows)]))
        else:
            pending = _PendingU(ctx, (D, R), u_r=scipy.sparse.hstack([u_local, coo_matrix((D, 1), dtype=np.float32)]))
    display("Normalizing by weights")
    display("The total rank before pruning is {}".format(R))
    lap("assembly", t0)
    return pending, _Columns(ranks, offsets, col_off_dev, w_dev, Rt, R, Rt + max(K, 0))


def _virtual_tiles(ctx, dist, tl, cols):
    """From here on a "tile" is a block of 64 component rows: tile t with rpad = 64 nvt rows becomes the nvt virtual tiles
    t nvt + h (same pixels, components 64 h .. 64 h + 63), in the same memory.  Column order, and with it every row
    index of the global stage, is unchanged; two virtual tiles of one tile overlap on all of its pixels."""
    nvt = tl.nvt
    if nvt == 1:
        return tl, cols
    ranks = np.clip(cols.ranks[:, None] - 64 * np.arange(nvt)[None, :], 0, 64).reshape(-1)
    offsets = np.concatenate([[0], np.cumsum(ranks)]).astype(np.int64)
    ranks_dev = _virtual_ranks(tl.ranks_dev, nvt)
    col_off_dev = _i32(ctx, offsets[:-1])
    pix_dev = tl.pix_dev.repeat_interleave(nvt, dim=0)
    tl = tl._replace(
        ranks_dev=ranks_dev, ut_dev=tl.ut_dev.view(tl.n_tiles * nvt, 64, tl.ut_dev.shape[2]),
        v_dev=None if tl.v_dev is None else tl.v_dev.view(tl.n_tiles * nvt, 64, tl.ldv),
        pix_c=np.repeat(tl.pix_c, nvt, axis=0), origins=np.repeat(np.asarray(tl.origins), nvt, axis=0), pix_dev=pix_dev,
        pix_loc_dev=tl.pix_loc_dev.repeat_interleave(nvt, dim=0) if dist.enabled else pix_dev,
        pairs=grid.virtual_pairs(tl.pairs, nvt), runs=[(lo * nvt, hi * nvt) for lo, hi in tl.runs],
        batches=[(lo * nvt, hi * nvt) for lo, hi in tl.batches], n_tiles=tl.n_tiles * nvt, t_lo=tl.t_lo * nvt, t_hi=tl.t_hi * nvt)
    return tl, cols._replace(ranks=ranks, offsets=offsets, col_off_dev=col_off_dev)


class _Weighted(NamedTuple):
    uw_dev: object        # U W: the tile components times the normalised pyramid weights
    pairs_dev: object
    origins_dev: object


def _weight_tiles(ctx, geom, tl, cols):
    torch = _torch()
    cumw_dev = _f32(ctx, tl.cumw.reshape(-1))
    uw_dev = torch.empty_like(tl.ut_dev)
    ctx.call("pmd_weight_tiles", ptr(tl.ut_dev), tl.ut_dev.shape[2], ptr(tl.pix_dev), geom.d, ptr(cols.w_dev), ptr(cumw_dev),
             ptr(tl.ranks_dev), ptr(uw_dev), tl.n_tiles)
    return _Weighted(uw_dev, _i32(ctx, tl.pairs), _i32(ctx, tl.origins))


class _Right(NamedTuple):
    right: object         # (Rc, m_cols) v_cropped = [tile traces ; background temporal basis], or its random sketch
    m_cols: int
    row_bounds: list      # rows of `right` (components) of every rank's tile run
    use_right: bool       # R > m_cols (decomposition.py:976): the mixing matrix stays factored
    col_sigma: object     # diagnostics: norm of every trace (tile sigma)


def _right_matrix(ctx, dist, tl, cols, pj_dev, K, crop, prune, seed, orthogonalizer, return_diagnostics):
    """v_cropped (decomposition.py:844, :932), the rank_prune sketch of it (prune = (rank_prune, rank_prune_factor)) and
    the rows of it a rank needs from the others."""
    torch = _torch()
    Rt, R, Rc, offsets = cols.Rt, cols.R, cols.Rc, cols.offsets
    t_lo, n_loc = tl.t_lo, tl.n_loc
    m_cols = crop
    vc = torch.zeros((Rc, m_cols), dtype=torch.float32, device=ctx.device)
    if n_loc > 0 and tl.batched:
        row = int(offsets[t_lo])
        for piece in tl.v_pieces:
            vc[row:row + piece.shape[0]] = piece
            row += piece.shape[0]
        tl.v_pieces.clear()     # lifetime: the pieces go once copied
    elif n_loc > 0:
        ctx.call("pmd_compact_rows", ptr(tl.v_dev[t_lo:]), tl.ldv, ptr(cols.col_off_dev[t_lo:]), ptr(tl.ranks_dev[t_lo:]), crop,
                 ptr(vc), m_cols, n_loc)
    row_bounds = [(int(offsets[lo]), int(offsets[hi])) for lo, hi in tl.runs]
    if K > 0:
        vc[Rt:Rt + K, :] = pj_dev[:, :crop]
    right = vc
    col_sigma = vc.norm(dim=1).cpu().numpy() if return_diagnostics else None
    rank_prune, rank_prune_factor = prune
    if rank_prune:
        if rank_prune_factor <= 0 or rank_prune_factor > 1:
            raise ValueError("Rank prune factor should be a value in the interval (0, 1]")
        min_dimension = min(R, crop)
        n_rand = int(min_dimension * rank_prune_factor)
        rand = torch.empty((crop, max(n_rand, 1)), dtype=torch.float32, device=ctx.device)
        ctx.call("pmd_rng_normal", seed, STREAM_PRUNE, 0, 0, 1, crop, n_rand, 0, ptr(rand), n_rand, 0)
        right = torch.empty((Rc, n_rand), dtype=torch.float32, device=ctx.device)
        ctx.call("pmd_gemm", 0, 0, Rc, n_rand, crop, 1.0, ptr(vc), m_cols, ptr(rand), n_rand, 0.0, ptr(right), n_rand)
        m_cols = n_rand
    use_right = R > m_cols  # decomposition.py:976 (R counts the placeholder column too)
    # Rows of `right` that live on other ranks.  Row-sharded Cholesky route: a rank applies the block-sparse Gram
    # matrix to its own tiles only and needs, besides its own rows, the rows of the foreign tiles that overlap
    # them (a halo of one or two tile rows on either side: tens of MB instead of the whole 2.2 GB matrix at
    # config 3).  Every other route is replicated and collects all rows.
    # collectives: exactly one of the two exchanges, the same one on every rank
    if dist.enabled and use_right and orthogonalizer in ("auto", "cholesky"):
        tile_owner = np.searchsorted(np.asarray([hi for _, hi in tl.runs]), np.arange(tl.n_tiles), side="right")
        needs = [[] for _ in range(dist.world)]
        pa, pb = tl.pairs[:, 0].astype(np.int64), tl.pairs[:, 1].astype(np.int64)
        for a_t, b_t in ((pa, pb), (pb, pa)):
            cross = tile_owner[a_t] != tile_owner[b_t]
            for rr in range(dist.world):
                for t in np.unique(b_t[cross & (tile_owner[a_t] == rr)]):
                    needs[rr].append((int(offsets[t]), int(offsets[t + 1])))
        dist.exchange_rows(right, row_bounds, [sorted(set(x for x in nd if x[1] > x[0])) for nd in needs])
    elif dist.enabled:
        dist.gather_runs(right, row_bounds)
    _dbg("v_cropped", vc)
    return _Right(right, m_cols, row_bounds, use_right, col_sigma)


class _ZBuilder:
    """Z = (U W)^T ((Y - mean) / std) over the whole movie (pmd_loader.py:316-346), for the resident plans (one launch,
    or one per batch of tiles) and the streamed one (pass 2 of the source).  Everything Z needs is captured here, once."""

    def __init__(self, ctx, dist, own, geom, movie, stats, std, tl, cols, uw_dev, K, lap):
        self.ctx, self.dist, self.own, self.movie, self.stats, self.tl, self.cols = ctx, dist, own, movie, stats, tl, cols
        self.uw_dev, self.K, self.lap, self.d, self.T = uw_dev, K, lap, geom.d, movie.T
        self.D = geom.D
        # single-copy plan: the filtered movie (+ the rank-K term in build); streamed: no movie copy at all (both None)
        self.src = std.xf if std.xs_full is None else std.xs_full
        self.has_full, self.pj_dev, self.ld_f, self.ld_T, self.all_frames = std.xs_full is not None, std.pj_dev, std.ld_f, std.ld_T, std.all_frames

    def _project_tiles(self, z, f0, src, ld, n, b0, nb, proj):
        """Columns [f0, f0 + n) of Z for the nb local tiles from b0: their traces on the n frames of src, compacted to the
        kept components (the rows of Z)."""
        ctx, tl, cols = self.ctx, self.tl, self.cols
        g0 = tl.t_lo + b0
        ctx.call("pmd_tiles_project_ranked", ptr(src), ld, n, ptr(tl.pix_loc_dev[b0:]), nb, self.d, ptr(self.uw_dev[g0:]),
                 self.uw_dev.shape[2], ptr(proj), ld, 2, ptr(tl.ranks_dev[g0:]))
        ctx.call("pmd_compact_rows", ptr(proj), ld, ptr(cols.col_off_dev[g0:]), ptr(tl.ranks_dev[g0:]), n, ptr(z.view(-1)[f0:]),
                 self.T, nb)

    def build(self, everywhere, bg_strip=None):
        """A rank projects the tiles of its own run (it holds no other pixels); everywhere=True then collects all rows on
        every rank (the replicated global stage), otherwise a rank keeps only its own rows (row-sharded stage).  The K
        background rows are filled on every rank.  bg_strip: (K x Rc) background rows of U^T U (single-copy plan)."""
        if self.movie.streamed:
            return self._build_streamed()
        torch = _torch()
        ctx, dist, own, tl, K, T, ld_T = self.ctx, self.dist, self.own, self.tl, self.K, self.T, self.ld_T
        Rt, offsets = self.cols.Rt, self.cols.offsets
        z = torch.zeros((self.cols.Rc, T), dtype=torch.float32, device=ctx.device)
        if tl.n_loc > 0 and tl.batched:
            for b0, b1_ in tl.batches:
                proj = torch.empty((b1_ - b0, 64, ld_T), dtype=torch.float32, device=ctx.device)
                self._project_tiles(z, 0, self.src, ld_T, T, b0, b1_ - b0, proj)
                del proj
        elif tl.n_loc > 0:
            if self.all_frames and tl.ldv == ld_T:
                proj = tl.v_dev     # same shape; the fit-frame traces are already compacted into v_cropped
            else:
                proj = torch.empty((tl.n_tiles, 64, ld_T), dtype=torch.float32, device=ctx.device)
            self._project_tiles(z, 0, self.src, ld_T, T, 0, tl.n_loc, proj[tl.t_lo:])
        if not self.has_full and K > 0:
            # (UW)^T X = (UW)^T X_f + ((UW)^T B) (B^T X): bg_strip[k][c] = (B^T U W)[k][c], pj_dev = B^T X
            lo_, hi_ = int(offsets[tl.t_lo]), int(offsets[tl.t_hi])
            if hi_ > lo_:
                ctx.call("pmd_gemm", 1, 0, hi_ - lo_, T, K, 1.0, ptr(bg_strip[:, lo_:]), bg_strip.shape[1], ptr(self.pj_dev),
                         self.ld_f, 1.0, ptr(z[lo_:]), T)
        if everywhere:
            dist.gather_runs(z, [(int(offsets[lo]), int(offsets[hi])) for lo, hi in tl.runs])
        if K > 0:
            if self.all_frames:
                z[Rt:Rt + K, :] = self.pj_dev[:, :T]
            else:
                pj_full = torch.zeros((K, ld_T), dtype=torch.float32, device=ctx.device)
                ws_ = ctx.workspace(ctx.lib.pmd_bg_project_workspace_bytes(own.O_hi - own.O_lo, T))
                ctx.call("pmd_bg_project", ptr(self.src[own.O_lo - own.P_lo:]), own.O_hi - own.O_lo, T, ld_T,
                         ptr(self.stats.basis_dev[own.O_lo:]), K, ptr(pj_full), ld_T, ptr(ws_), ws_.numel())
                dist.all_reduce(pj_full)
                z[Rt:Rt + K, :] = pj_full[:, :T]
        return z

    def _build_streamed(self):
        """Pass 2 of the streamed mode: Z[:, t0:t0+n] = (U W)^T X and B^T X of every block of frames, standardised
        from the source as it is read again (single process: every tile, every pixel)."""
        torch = _torch()
        ctx, movie, tl, K, Rt, T = self.ctx, self.movie, self.tl, self.K, self.cols.Rt, self.T
        mean_dev, std_dev, basis_dev = self.stats
        t_z = time.perf_counter()
        z = torch.zeros((self.cols.Rc, T), dtype=torch.float32, device=ctx.device)
        tile_runs = (tl.batches if tl.batched else [(0, tl.n_loc)]) if tl.n_loc > 0 else []
        ld_b = int(ctx.lib.pmd_time_ld(movie.project_frames))
        proj = torch.empty((max([b - a for a, b in tile_runs] + [1]), 64, ld_b), dtype=torch.float32, device=ctx.device)
        pj_b = torch.zeros((K, ld_b), dtype=torch.float32, device=ctx.device) if K > 0 else None
        ws_ = ctx.workspace(ctx.lib.pmd_bg_project_workspace_bytes(self.D, movie.project_frames)) if K > 0 else None

        def on_block(xs, ld, f0, n):      # callback of the movie pass
            for b0, b1_ in tile_runs:
                self._project_tiles(z, f0, xs, ld, n, b0, b1_ - b0, proj)
            if K > 0:
                ctx.call("pmd_bg_project", ptr(xs), self.D, n, ld, ptr(basis_dev), K, ptr(pj_b), ld_b, ptr(ws_), ws_.numel())
                z[Rt:Rt + K, f0:f0 + n] = pj_b[:, :n]

        movie.project(mean_dev, std_dev, on_block)
        self.lap("stream_projection", t_z)
        return z


class _Mixing(NamedTuple):
    """The mixing matrix P with (U P)^T (U P) = I, rp columns: dense (P_dev, the R <= frames route) or factored,
    P = right[:, :m_used] Et[:rp, :m_used]^T (Cholesky route: chol_ok; else the eigenvector route)."""
    rp: int
    P_dev: object = None
    Et_dev: object = None
    m_used: int = 0
    chol_ok: bool = False
    null_tail: bool = False   # Cholesky route: row m_used of Et is the kept null direction, carried next to the joint SVD
    null_info: dict = {}      # its pivot level and the coupling left out (diagnostics); never mutated in place
    shard: bool = False       # rows of right / Z / R split over the ranks (Cholesky route only)
    row_lo: int = 0           # rows owned by this rank
    row_hi: int = 0
    Z: object = None          # Z and W1 = M^T Z, when the Cholesky route already formed them next to its factorisation
    W1: object = None
    bg_strip: object = None   # (K x Rc) background rows of U^T U (single-copy plan: the rank-K term of the projection)


class _BlockGram:
    """G = U^T U kept block-sparse (tile-pair blocks, background blocks and the background strip) and its product with
    the columns of `right`."""

    def __init__(self, ctx, dist, geom, tl, cols, wt, rt, basis_dev, K):
        torch = _torch()
        self.ctx, self.dist, self.tl, self.cols, self.rt, self.K = ctx, dist, tl, cols, rt, K
        Rt, Rc, n_tiles = cols.Rt, cols.Rc, tl.n_tiles
        n_pairs = tl.pairs.shape[0]
        self.gblk = torch.empty((max(n_pairs, 1), 64, 64), dtype=torch.float32, device=ctx.device)
        self.gbg = torch.zeros((max(1, (max(K, 0) + 63) // 64) * n_tiles, 64, 64), dtype=torch.float32, device=ctx.device)
        self.gstrip = torch.zeros((max(K, 1), Rc), dtype=torch.float32, device=ctx.device)
        ctx.call("pmd_gram_blocks", ptr(wt.uw_dev), wt.uw_dev.shape[2], geom.b1, geom.b2, ptr(tl.pix_dev), ptr(wt.pairs_dev),
                 n_pairs, ptr(wt.origins_dev), ptr(cols.col_off_dev), ptr(tl.ranks_dev), n_tiles, Rt, ptr(basis_dev), geom.D,
                 max(K, 0), ptr(self.gblk), ptr(self.gbg), ptr(self.gstrip), Rc)
        nbr_ptr, nbr = grid.neighbour_lists(tl.pairs, cols.ranks, cols.offsets[:-1], n_tiles, Rt, max(K, 0))
        self.nbr_ptr_dev, self.nbr_dev = _i32(ctx, nbr_ptr), _i32(ctx, nbr)

    def apply(self, ncols, GM, shard):
        """GM[:, :ncols] = G right[:, :ncols]: block rows for the tiles of this rank (all tiles when not sharded); the K
        background rows come from one small GEMM inside the call (every rank forms them, only their owner uses them)."""
        torch = _torch()
        ctx, dist, tl, cols, K = self.ctx, self.dist, self.tl, self.cols, self.K
        right, m_cols, row_bounds = self.rt.right, self.rt.m_cols, self.rt.row_bounds
        Rt, Rc = cols.Rt, cols.Rc
        if tl.n_loc > 0 or not shard:
            a0, an = (tl.t_lo, tl.n_loc) if shard else (0, tl.n_tiles)
            ctx.call("pmd_gram_apply", ptr(self.gblk), ptr(self.gbg), ptr(self.gstrip), Rc, ptr(self.nbr_ptr_dev[a0:]),
                     ptr(self.nbr_dev), ptr(cols.col_off_dev[a0:]), ptr(tl.ranks_dev[a0:]), an, Rt, max(K, 0),
                     int(cols.ranks.max()) if tl.n_tiles else 0, ptr(right), m_cols, ncols, ptr(GM), m_cols)
        if shard and K > 0:
            # The background rows of G M are sums over ALL rows of `right`; a rank holds its own rows and a halo
            # only.  Every rank contributes the product over the rows it owns (the last one also the background
            # columns), the K x ncols partials are all-reduced, their owner (the last rank) keeps the result.
            part = torch.zeros((K, ncols), dtype=torch.float32, device=ctx.device)
            lo_, hi_ = row_bounds[dist.rank][0], (Rc if dist.rank == dist.world - 1 else row_bounds[dist.rank][1])
            if hi_ > lo_:
                ctx.call("pmd_gemm", 0, 0, K, ncols, hi_ - lo_, 1.0, ptr(self.gstrip[:, lo_:]), Rc, ptr(right[lo_:]), m_cols, 0.0,
                         ptr(part), ncols)
            dist.all_reduce(part)
            GM[Rt:Rt + K, :ncols] = part


def _householder(ctx, right, Rc, m_cols, hv_dev, y_dev):
    """right <- right H, H = I - 2 h h^T (an involution: the same call undoes it)."""
    ctx.call("pmd_gemm", 0, 0, Rc, 1, m_cols, 1.0, ptr(right), m_cols, ptr(hv_dev), 1, 0.0, ptr(y_dev), 1)
    ctx.call("pmd_gemm", 0, 0, Rc, m_cols, 1, -2.0, ptr(y_dev), 1, ptr(hv_dev), m_cols, 1.0, ptr(right), m_cols)


def _kept_null_pivot(Et_dev, m_eff, tr_c_dev):
    """Cholesky route, null_directions="keep": is the last pivot (the rotated-in constant vector) really at rounding
    level?  Returns (split it off next to the joint SVD?, null_info); floors an accidentally tiny pivot in Et."""
    # (with a large mean / noise ratio the fp32 centring leaves the constant vector a small but resolved
    # direction; splitting it off would then drop real signal.)  Et[m-1][m-1] = 1 / sqrt(|pivot|); compared with the mean
    # diagonal of C.
    piv = 1.0 / max(float(Et_dev[m_eff - 1, m_eff - 1].item()) ** 2, 1e-300)
    null_pivot_rel = piv / max(float(tr_c_dev.item()) / m_eff, 1e-300)
    # The pivot of a null direction is rounding noise and can come out accidentally tiny (3e-12 of the mean
    # diagonal seen: the kept direction was then scaled up 5e5 times and led the spectrum with 18 x s_1).
    # The reference's fp32 eigensolver returns |lambda| ~ eps32 lambda_max for such a direction, never less:
    # the pivot is floored at eps32 trace(C) / 4 (lambda_max <= trace), which bounds the amplification the
    # same way (the last row of Et is linear in 1 / sqrt(pivot)).
    floor_rel = 1.1920929e-07 * m_eff / 4.0
    if null_pivot_rel < floor_rel:
        Et_dev[m_eff - 1, :m_eff] *= math.sqrt(null_pivot_rel / floor_rel)
    # The last row of Et is the kept numerically null direction (scale 1 / sqrt(|last pivot|), as the
    # reference's 1 / sqrt(|lambda|), decomposition.py:984-996).  Its coupling to the other directions is
    # rounding noise, so it is carried as one extra component next to the SVD of the leading
    # m - 1 directions (whose Et block is exactly the Cholesky inverse of the deflated matrix)
    # instead of through it, where its huge coefficients would amplify rounding errors into every
    # other component.
    return (null_pivot_rel <= max(NULL_PIVOT_REL, 8.0 * floor_rel),
            {"pivot_rel": null_pivot_rel, "pivot_floor_rel": floor_rel})


def _cholesky_attempt(ctx, dist, gram, rt, zb, GM, Et_dev, Rc, T, rows, shard, rotate, keep_null, lap, t0):
    """Et = inverse Cholesky factor of C = right^T G right, with Z = (UW)^T Y and W1 = right^T Z formed next to it.
    rotate: the constant vector is a numerically null right vector - rotate it into the last column first.
    Returns (ok, m_eff, tr_c_dev or None, Z, W1, (hv_dev, y_dev) or None, t0 of the running "orthogonalize" lap);
    Z and W1 are None when C turned out not positive definite."""
    torch = _torch()
    lib = ctx.lib
    right, m_cols = rt.right, rt.m_cols
    row_lo, row_hi = rows
    m_eff = m_cols
    abs_last = 0
    rotation = None
    if rotate:
        # Every standardised trace sums to ~0 over the frames it was centred on (all of them: crop == T),
        # so the constant vector is a numerically null right vector of v_cropped.  Rotate it into the
        # last column (Householder H, H e_m = 1/sqrt(m)): the leading block of C is then well
        # conditioned and the null direction sits in the last pivot.  "keep" (the reference's rule:
        # |lambda| of a numerically null direction is kept, decomposition.py:984-988): the last pivot
        # enters through its absolute value; "drop": the column is dropped (one component fewer).
        nhat = np.full(m_cols, 1.0 / math.sqrt(m_cols))
        hv = -nhat
        hv[-1] += 1.0
        hv /= np.linalg.norm(hv)
        rotation = (_f32(ctx, hv), torch.empty((Rc, 1), dtype=torch.float32, device=ctx.device))
        _householder(ctx, right, Rc, m_cols, *rotation)
        if keep_null:
            abs_last = 1
        else:
            m_eff = m_cols - 1
    gram.apply(m_eff, GM, shard)
    ok_c = c_i(0)
    # C = right[rows]^T GM[rows] (summed over the ranks when the rows are sharded)
    if shard:
        Et_dev.zero_()
    nrow = row_hi - row_lo
    Mt_buf = None
    if nrow > 0:
        # pmd_gram_mtgm writes the transposed copy of its M rows at the start of its workspace; handing it a
        # buffer of our own keeps that copy for the M^T Z product below (one transpose and, at BASELINE
        # config 5, 20 GB fewer than a second copy).  Workspaces: an allocation of its own, because the shared
        # ctx.workspace is replaced by the requests made while Z is built.
        Mt_buf = torch.empty((lib.pmd_gram_mtgm_workspace_bytes(nrow, m_eff) + 3) // 4, dtype=torch.float32, device=ctx.device)
        ctx.call("pmd_gram_mtgm", ptr(right[row_lo:]), nrow, m_eff, m_cols, ptr(GM[row_lo:]), m_cols,
                 ptr(Et_dev), m_cols, ptr(Mt_buf), Mt_buf.numel() * 4)
    dist.all_reduce(Et_dev)
    tr_c_dev = Et_dev.diagonal()[:m_eff].sum() if abs_last else None   # scale of C for the null-pivot test
    # Streams: the Cholesky step (C -> Et) is a chain of small latency-bound launches; the V projection
    # Z = (UW)^T Y and the large product M^T Z do not depend on it.  Event on main -> Z and M^T Z enqueued on
    # main -> the Cholesky step on the side stream behind the event -> main waits -> ctx.sync().
    main = torch.cuda.current_stream(ctx.device)
    ev_c = torch.cuda.Event()
    ev_c.record(main)
    lap("orthogonalize", t0)
    t0 = time.perf_counter()
    Z = zb.build(everywhere=not shard, bg_strip=gram.gstrip)
    W1 = torch.zeros((m_eff, T), dtype=torch.float32, device=ctx.device)
    if nrow > 0:
        ld_mt = int(lib.pmd_gram_mtgm_ld(nrow))   # (rows of the transposed copy are padded to 64 floats)
        ctx.call("pmd_gemm", 0, 0, m_eff, T, nrow, 1.0, ptr(Mt_buf), ld_mt, ptr(Z[row_lo:]), T, 0.0, ptr(W1), T)
    lap("v_projection", t0)
    t0 = time.perf_counter()
    # (driving the side stream from a helper thread, so that the chain is enqueued before the blocking read-back
    # inside the M^T Z product, was tried: no gain at config 3 - the chain is bound by CU availability next to
    # the product, not by when it is enqueued - and erratic 40-70 ms waits at config 2; not kept)
    sc = ctx.side()
    sc.stream.wait_event(ev_c)
    with torch.cuda.stream(sc.stream):
        ws2 = sc.workspace(lib.pmd_chol_inverse_workspace_bytes(m_eff))
        sc.call("pmd_chol_inverse", ptr(Et_dev), m_eff, m_cols, abs_last, C.byref(ok_c), ptr(ws2), ws2.numel())
    ev_e = torch.cuda.Event()
    ev_e.record(sc.stream)
    main.wait_event(ev_e)
    ctx.sync()
    Mt_buf = None            # lifetime: the transposed copy goes after M^T Z
    ok = bool(ok_c.value)
    if ok:
        dist.all_reduce(W1)
    else:
        Z = W1 = None        # eigenvector route: full Z, M^T Z inside pmd_projected_svd_factored
    return ok, m_eff, tr_c_dev, Z, W1, rotation, t0


def _eigenvector_fallback(ctx, dist, gram, rt, GM, Et_dev, Rc, rotation, shard):
    """The reference's eigendecomposition of C (decomposition.py:984-996), replicated on every rank.  Returns rp."""
    right, m_cols = rt.right, rt.m_cols
    if rotation is not None:
        # Undo the rotation (H is an involution).  With the null direction isolated in the last column, the
        # eigensolver returns an eigenvalue for it that is orders of magnitude below the rounding level of
        # the unrotated matrix, and the reference's 1 / sqrt(|lambda|) rule then scales that direction up
        # until it swamps every other component (seen in the seeded fuzz: mean squared residual 1400
        # instead of 1.3).  Unrotated, the route is exactly the eigenvector route the caller can also ask for.
        _householder(ctx, right, Rc, m_cols, *rotation)
    if shard:
        dist.gather_runs(right, rt.row_bounds)   # collectives: only the halo rows were exchanged so far
    gram.apply(m_cols, GM, False)
    ws = ctx.workspace(ctx.lib.pmd_orthogonalize_factored_workspace_bytes(m_cols))
    rp_c = c_i(0)
    ctx.call("pmd_orthogonalize_factored", ptr(right), Rc, m_cols, m_cols, ptr(GM), m_cols, ptr(Et_dev), m_cols,
             C.byref(rp_c), ptr(ws), ws.numel())
    return int(rp_c.value)


def _factored_mixing(ctx, dist, geom, tl, cols, wt, rt, zb, basis_dev, K, T, route, lap, t0):
    """R > frames: P = right E / sqrt(lambda) stays factored and G = U^T U block-sparse.
    route = (orthogonalizer, keep the null direction?, rotate the constant vector?).  Returns (_Mixing, t0)."""
    torch = _torch()
    orthogonalizer, keep_null, rotate = route
    Rc, m_cols = cols.Rc, rt.m_cols
    gram = _BlockGram(ctx, dist, geom, tl, cols, wt, rt, basis_dev, K)
    GM = torch.empty((Rc, m_cols), dtype=torch.float32, device=ctx.device)
    Et_dev = torch.empty((m_cols, m_cols), dtype=torch.float32, device=ctx.device)
    # Rows of `right`, GM, Z and R owned by this rank: the components of its tile run; the last rank
    # also owns the K background rows.  Single process: everything.
    row_lo, row_hi = int(cols.offsets[tl.t_lo]), int(cols.offsets[tl.t_hi])
    if dist.rank == dist.world - 1:
        row_hi = Rc
    shard = dist.enabled
    mix = None
    rotation = None
    if orthogonalizer in ("auto", "cholesky"):
        ok, m_eff, tr_c_dev, Z, W1, rotation, t0 = _cholesky_attempt(
            ctx, dist, gram, rt, zb, GM, Et_dev, Rc, T, (row_lo, row_hi), shard, rotate, keep_null, lap, t0)
        if ok:
            null_tail, null_info = _kept_null_pivot(Et_dev, m_eff, tr_c_dev) if tr_c_dev is not None else (False, {})
            rp = m_eff - 1 if null_tail else m_eff
            mix = _Mixing(rp, Et_dev=Et_dev, m_used=rp, chol_ok=True, null_tail=null_tail, null_info=null_info, shard=shard,
                          row_lo=row_lo, row_hi=row_hi, Z=Z, W1=W1, bg_strip=gram.gstrip)
        elif orthogonalizer == "cholesky":
            raise PMDLibraryError("orthogonalizer='cholesky': U^T U restricted to the right matrix is not positive definite")
    if mix is None:
        rp = _eigenvector_fallback(ctx, dist, gram, rt, GM, Et_dev, Rc, rotation, shard)
        mix = _Mixing(rp, Et_dev=Et_dev, m_used=m_cols, row_hi=Rc, bg_strip=gram.gstrip)
    return mix, t0       # lifetime: GM and the Gram blocks go with this frame; only the background strip is handed on


def _dense_mixing(ctx, geom, tl, cols, wt, rt, basis_dev, K, single_copy):
    """R <= frames (decomposition.py:976-1010): dense G = U^T U and its eigendecomposition."""
    torch = _torch()
    Rt, Rc = cols.Rt, cols.Rc
    G = torch.empty((Rc, Rc), dtype=torch.float32, device=ctx.device)
    ctx.call("pmd_gram_u", ptr(wt.uw_dev), wt.uw_dev.shape[2], geom.b1, geom.b2, ptr(tl.pix_dev), ptr(wt.pairs_dev),
             tl.pairs.shape[0], ptr(wt.origins_dev), ptr(cols.col_off_dev), ptr(tl.ranks_dev), tl.n_tiles, Rt, ptr(basis_dev),
             geom.D, max(K, 0), ptr(G), Rc)
    _dbg("G", G)
    bg_strip = G[Rt:Rt + K, :].clone() if (K > 0 and single_copy) else None   # G is overwritten by the eigendecomposition
    P_dev, rp = _orthogonalize(ctx, G, Rc, None, rt.m_cols, rt.m_cols)
    return _Mixing(rp, P_dev, row_hi=Rc, bg_strip=bg_strip)    # lifetime: G goes with this frame


R_DOWNLOAD_BLOCKS = 4     # row blocks in which a large R is formed and downloaded, one behind the other


def _svd_by_frame_columns(ctx, dist, mix, m_cols, T, s_out, Vt_out, X1, Vp):
    """Row-sharded Cholesky route.  The frames x frames products of the last stage by FRAME COLUMNS (round 3): rank r
    forms its T / N columns of Vp = Et W1 and their Gram matrix; the partial Gram matrices are all-reduced (one more
    m x m exchange); the eigensolver runs replicated; every rank then forms its columns of Vt, which travel to rank 0."""
    torch = _torch()
    rp, m_used, Et_dev = mix.rp, mix.m_used, mix.Et_dev
    cparts = tile_partition(T, dist.world)
    c0, c1 = cparts[dist.rank]
    nc = c1 - c0
    ldc = _round_up(rp, 4)
    Vp_r = torch.empty((rp, max(nc, 1)), dtype=torch.float32, device=ctx.device)
    Cg = torch.zeros((rp, ldc), dtype=torch.float32, device=ctx.device)
    ctx.call("pmd_psvd_vp_gram", ptr(Et_dev), rp, m_used, m_cols, ptr(mix.W1.view(-1)[c0:]), nc, T, 1 if mix.chol_ok else 0,
             ptr(Vp_r), max(nc, 1), ptr(Cg), ldc)
    dist.all_reduce(Cg)
    Wmat = torch.empty((rp, rp), dtype=torch.float32, device=ctx.device)
    Vt_r = torch.empty((rp, max(nc, 1)), dtype=torch.float32, device=ctx.device)
    ws = ctx.workspace(ctx.lib.pmd_psvd_finish_workspace_bytes(rp))
    ctx.call("pmd_psvd_finish", ptr(Cg), ldc, rp, ptr(Vp_r), nc, max(nc, 1), ptr(Wmat), rp, ptr(s_out), ptr(Vt_r),
             max(nc, 1), ptr(ws), ws.numel())
    ctx.call("pmd_gemm", 1, 0, m_used, rp, rp, 1.0, ptr(Et_dev), m_cols, ptr(Wmat), rp, 0.0, ptr(X1), rp)
    ctx.sync()
    blocks = dist.gather_blocks_to_root(Vt_r[:, :nc].contiguous(), [(rp, b_ - a_) for a_, b_ in cparts])
    if blocks is not None:
        for (a_, b_), blk in zip(cparts, blocks):
            if b_ > a_:
                Vt_out[:rp, a_:b_] = blk
    if Vp is not None:      # diagnostics only: every rank gets the whole V = P^T Z (a sum of disjoint column blocks)
        Vp.zero_()
        if nc > 0:
            Vp[:, c0:c1] = Vp_r[:, :nc]
        dist.all_reduce(Vp)


def _null_component(ctx, mix, T, nk, s_out, Vt_out, want_coupling):
    """The kept null direction: P column = right Et[m-1, :]^T, V row = Et[m-1, :] (right^T Z), its own singular triple
    (s = |V row|, Vt = V row / s, R column = P column) appended as the last component.  Returns (Et row, coupling)."""
    torch = _torch()
    m_full = mix.m_used + 1
    et_row = mix.Et_dev[m_full - 1, :m_full]
    v_null = Vt_out[nk:nk + 1]
    ctx.call("pmd_gemm", 0, 0, 1, T, m_full, 1.0, ptr(et_row), m_full, ptr(mix.W1), T, 0.0, ptr(v_null), T)
    # the joint SVD of the reference would deflate this row against the other right vectors: do the same
    # (two passes of classical Gram-Schmidt against the orthonormal rows of Vt), so that Vt stays orthonormal
    coef = torch.empty((nk,), dtype=torch.float32, device=ctx.device)
    for gs_pass in range(2):
        ctx.call("pmd_gemm", 0, 0, nk, 1, T, 1.0, ptr(Vt_out), T, ptr(v_null), 1, 0.0, ptr(coef), 1)
        if gs_pass == 0 and want_coupling:
            coef_norm = coef.norm()
        ctx.call("pmd_gemm", 0, 0, 1, T, nk, -1.0, ptr(coef), nk, ptr(Vt_out), T, 1.0, ptr(v_null), T)
    s_null = v_null.norm()
    coupling = None
    if want_coupling:
        # what the split-off leaves out of R diag(s) Vt: p_null (coef^T Vt), relative to the null row itself
        coupling = float((coef_norm / torch.clamp(s_null, min=1e-30)).item())
    s_out[nk:nk + 1] = s_null
    v_null.div_(torch.where(s_null == 0, torch.ones_like(s_null), s_null))
    return et_row, coupling


def _download_rows(main, side, r_host, R_out, lo, hi):
    """Streams: rows [lo, hi) of R go to the host on the side stream, behind an event recorded on main."""
    torch = _torch()
    ev = torch.cuda.Event()
    ev.record(main)
    side.wait_event(ev)
    with torch.cuda.stream(side):
        r_host[lo:hi].copy_(R_out[lo:hi], non_blocking=True)


def _form_r_and_download(ctx, dist, tl, cols, rt, mix, shard, outs, X1, et_row, zero_copy, split_gemm, extra_row):
    """R = right X1 in row blocks; s, Vt and every finished block go to the host on a side stream while the next block
    is computed (2.6 GB of results, ~45 ms of PCIe time otherwise serial).  Returns host (R, s, Vt) on rank 0, else None."""
    torch = _torch()
    R_out, s_out, Vt_out = outs
    right, m_cols, Rc, rp, m_used = rt.right, rt.m_cols, cols.Rc, mix.rp, mix.m_used
    nk, nko = rp, s_out.shape[0]
    main = torch.cuda.current_stream(ctx.device)
    side = _side_stream(ctx.device)
    root = dist.rank == 0
    r_host = None
    if root:
        r_host = torch.empty((Rc + extra_row, nko), dtype=torch.float32, pin_memory=True)
        s_host = torch.empty((nko,), dtype=torch.float32, pin_memory=True)
        vt_host = torch.empty((nko, Vt_out.shape[1]), dtype=torch.float32, pin_memory=True)
        if extra_row:
            r_host[Rc:].zero_()
        ev = torch.cuda.Event()
        ev.record(main)
        side.wait_event(ev)      # streams: s and Vt leave behind an event recorded on main
        with torch.cuda.stream(side):
            s_host.copy_(s_out, non_blocking=True)
            vt_host.copy_(Vt_out, non_blocking=True)
    download = functools.partial(_download_rows, main, side, r_host, R_out)
    # R = right X1.  On rank 0 the GEMM writes its rows straight into the pinned host array (zero copy: the
    # tile stores go over PCIe while the product is still being computed - 83 ms for the 2.2 GB at config 3
    # against 75 ms into HBM plus 39 ms of download, scripts/gemm_probe3.hip).
    r_lo, r_hi = (mix.row_lo, mix.row_hi) if shard else (0, Rc)
    if r_hi > r_lo:
        dst = r_host[r_lo:] if (root and zero_copy) else R_out[r_lo:]
        if mix.null_tail:
            # last column first (a small product and, on the zero-copy path, a blocking copy: before the large
            # asynchronous GEMM is enqueued, which writes the other columns of the same rows)
            m_full = m_used + 1
            p_null = torch.empty((r_hi - r_lo, 1), dtype=torch.float32, device=ctx.device)
            ctx.call("pmd_gemm", 0, 0, r_hi - r_lo, 1, m_full, 1.0, ptr(right[r_lo:]), m_cols, ptr(et_row), 1, 0.0,
                     ptr(p_null), 1)
            if root and zero_copy:
                r_host[r_lo:r_hi, nk:nko].copy_(p_null)
            else:
                R_out[r_lo:r_hi, nk:nko] = p_null
        if root and not zero_copy and split_gemm and (r_hi - r_lo) * nk * 4 >= 2 ** 30:
            step_r = max(4096, -(-(r_hi - r_lo) // R_DOWNLOAD_BLOCKS // 256) * 256)
            for b_lo in range(r_lo, r_hi, step_r):
                b_hi = min(r_hi, b_lo + step_r)
                ctx.call("pmd_gemm", 0, 0, b_hi - b_lo, nk, m_used, 1.0, ptr(right[b_lo:]), m_cols, ptr(X1), rp, 0.0,
                         ptr(R_out[b_lo:]), nko)
                download(b_lo, b_hi)
        else:
            ctx.call("pmd_gemm", 0, 0, r_hi - r_lo, nk, m_used, 1.0, ptr(right[r_lo:]), m_cols, ptr(X1), rp, 0.0,
                     ptr(dst), nko)
            if root and not zero_copy:
                download(r_lo, r_hi)
    if shard:
        # collectives: the other ranks' row blocks of R travel to rank 0 and are downloaded as they arrive
        ctx.sync()
        bounds = [(int(cols.offsets[lo]), Rc if rr == dist.world - 1 else int(cols.offsets[hi]))
                  for rr, (lo, hi) in enumerate(tl.runs)]
        dist.gather_rows_to_root(R_out, bounds, on_block=download if root else None)
    side.synchronize()
    return (r_host.numpy(), s_host.numpy(), vt_host.numpy()) if root else None


def _factored_svd(ctx, dist, tl, cols, rt, mix, Z, T, shard, extra_row, Vp):
    """V = P^T Z and the final SVD for the factored P with rp <= T.  Returns (host (R, s, Vt) or None, null_info)."""
    torch = _torch()
    lib = ctx.lib
    Rc, m_cols, rp, m_used = cols.Rc, rt.m_cols, mix.rp, mix.m_used
    nk = rp
    nko = nk + (1 if mix.null_tail else 0)   # components in the outputs
    # device copy of R only where rows are exchanged between ranks; rank 0's own rows go straight to the host
    # Zero copy only for the large case it was measured on: for small outputs rocBLAS may pick split-K kernels
    # that read-modify-write C, which is ruinous across PCIe (58 ms instead of 1 ms at 5015 x 1999).
    # (not when the product runs as fp16-piece products, gemm_f16x2.hip: its three passes accumulate into C, which
    # must then live in HBM; R is formed in row blocks there, each downloaded while the next is computed)
    split_gemm = bool(lib.pmd_gemm_split_active(ctx.handle, min(Rc, 16384), nk, m_used))
    zero_copy = (not shard or dist.rank == 0) and m_used >= 8192 and Rc * nk * 4 >= 2 ** 30 and not split_gemm
    R_out = torch.empty((Rc, nko), dtype=torch.float32, device=ctx.device) if (shard or not zero_copy) else None
    s_out = torch.empty((nko,), dtype=torch.float32, device=ctx.device)
    Vt_out = torch.empty((nko, T), dtype=torch.float32, device=ctx.device)
    X1 = torch.empty((m_used, rp), dtype=torch.float32, device=ctx.device)
    # W1 = M^T Z was formed next to the Cholesky step (summed over the ranks when the rows are sharded);
    # None on the eigenvector route (formed inside the call)
    if shard:
        _svd_by_frame_columns(ctx, dist, mix, m_cols, T, s_out, Vt_out, X1, Vp)
    else:
        ws = ctx.workspace(lib.pmd_projected_svd_factored_workspace_bytes(Rc, m_used, rp, T))
        ctx.call("pmd_projected_svd_factored", ptr(rt.right), Rc, m_used, m_cols, ptr(mix.Et_dev), rp, m_cols, ptr(Z), T, T,
                 None, nk, ptr(s_out), ptr(Vt_out), T, ptr(Vp), T, ptr(X1), ptr(mix.W1), 1 if mix.chol_ok else 0, ptr(ws),
                 ws.numel())
    et_row, null_info = None, mix.null_info
    if mix.null_tail:
        et_row, coupling = _null_component(ctx, mix, T, nk, s_out, Vt_out, Vp is not None)
        if coupling is not None:
            null_info = dict(null_info, coupling_rel=coupling)
    hosts = _form_r_and_download(ctx, dist, tl, cols, rt, mix, shard, (R_out, s_out, Vt_out), X1, et_row, zero_copy, split_gemm,
                                 extra_row)
    return hosts, null_info


def _dense_svd(ctx, cols, rt, mix, Z, T, Vp):
    """V = P^T Z and its SVD with a dense P.  Returns (device (R, s, Vt), Vp)."""
    torch = _torch()
    Rc, m_cols, rp, P_dev = cols.Rc, rt.m_cols, mix.rp, mix.P_dev
    if P_dev is None:  # factored P with R' > T (rank_prune corner): materialise P = right Et^T
        P_dev = torch.empty((Rc, m_cols), dtype=torch.float32, device=ctx.device)
        ctx.call("pmd_gemm", 0, 1, Rc, rp, mix.m_used, 1.0, ptr(rt.right), m_cols, ptr(mix.Et_dev), m_cols, 0.0, ptr(P_dev), m_cols)
    ldp = P_dev.shape[1]
    if Vp is None:
        Vp = torch.empty((rp, T), dtype=torch.float32, device=ctx.device)
    ctx.call("pmd_gemm", 1, 0, rp, T, Rc, 1.0, ptr(P_dev), ldp, ptr(Z), T, 0.0, ptr(Vp), T)
    return _projected_svd_dev(ctx, P_dev, Rc, ldp, Vp, rp, T, T), Vp


def _host_results(hosts, outs, null_tail, extra_row, root_only):
    """(r, s, vt) on the host, `s` descending and without exactly-zero components; None x 3 where the results live on rank 0."""
    if root_only:
        return None, None, None
    if hosts is not None:
        r_mat, s, vt = hosts
    else:
        r_mat, s, vt = (_to_host(t) for t in outs)
        if extra_row:
            r_mat = np.concatenate([r_mat, np.zeros((1, r_mat.shape[1]), dtype=r_mat.dtype)], axis=0)
    if null_tail and len(s) > 1 and s[-1] > s[-2]:
        # the appended component is normally the smallest; keep `s` descending in any case (as svd returns it)
        order_s = np.argsort(-s, kind="stable")
        r_mat, s, vt = r_mat[:, order_s], s[order_s], vt[order_s]
    good_components = s != 0
    if not np.all(good_components):
        r_mat = r_mat[:, good_components]
        s = s[good_components]
        vt = vt[good_components, :]
    return r_mat, s, vt


def _statistic_images(ctx, dist, own, geom, stats):
    """Mean and noise-level images of the whole field of view (every rank contributes its owned pixels)."""
    torch = _torch()
    mean_dev, std_dev = stats.mean_dev, stats.std_dev
    if dist.enabled:
        mean_all = torch.zeros(geom.D, dtype=torch.float32, device=ctx.device)
        std_all = torch.zeros(geom.D, dtype=torch.float32, device=ctx.device)
        mean_all[own.O_lo:own.O_hi] = mean_dev[own.O_lo - own.P_lo:own.O_hi - own.P_lo]
        std_all[own.O_lo:own.O_hi] = std_dev[own.O_lo - own.P_lo:own.O_hi - own.P_lo]
        dist.gather_runs(mean_all, own.owned)      # collectives: mean, then std
        dist.gather_runs(std_all, own.owned)
        mean_dev, std_dev = mean_all, std_all
    return mean_dev.cpu().numpy().reshape(geom.d1, geom.d2), std_dev.cpu().numpy().reshape(geom.d1, geom.d2)


def _release(ctx, own_ctx):
    try:
        ctx.sync()
    except Exception:
        pass
    ctx.release_pinned()
    try:
        # scratch of the large products: kept between calls up to 8 GiB, larger ones are returned to the device
        ctx.call("pmd_scratch_trim", 8 << 30)
    except Exception:
        pass
    if own_ctx:
        ctx.release_workspace()
        ctx.close()


def localmd_decomposition(
    dataset_obj,
    block_sizes: tuple,
    frame_range: int,
    max_components: int = 50,
    background_rank: int = 15,
    sim_conf: int = 5,
    frame_batch_size: int = 10000,
    dtype: str = "float32",
    num_workers: int = 0,
    pixel_batch_size: int = 5000,
    max_consecutive_failures=1,
    rank_prune: bool = False,
    rank_prune_factor: float = 0.33,
    temporal_avg_factor: int = 10,
    spatial_avg_factor: int = 2,
    order: str = "F",
    window_chunks: Optional[int] = None,
    compute_normalizer: bool = True,
    pixel_weighting: Optional[np.ndarray] = None,
    spatial_denoiser: Optional[Callable] = None,
    temporal_denoiser: Optional[Callable] = None,
    *,
    seed: Optional[int] = None,
    device: Optional[int] = None,
    thresholds=None,
    sim_iters: int = 250,
    orthogonalizer: str = "auto",
    null_directions: str = "keep",
    null_cutoff: float = 0.0,
    single_copy: Optional[bool] = None,
    tile_batch_bytes: int = 24 << 30,
    distributed: bool = False,
    return_diagnostics: bool = False,
    ctx: Optional[Context] = None,
    stream: Optional[bool] = None,
):
    torch = _torch()
    _check_options(dataset_obj, dtype, spatial_denoiser, temporal_denoiser, order, orthogonalizer, null_directions, stream,
                   distributed)
    t_start = time.perf_counter()
    T, d1, d2 = (int(x) for x in dataset_obj.shape)
    grid.check_fov_size((d1, d2))
    own_ctx = ctx is None
    if own_ctx:
        ctx = Context(0 if device is None else device)
    try:
        lap = _Laps(ctx, return_diagnostics)
        # decomposition.py:984-996 keeps every direction of the orthogonalising eigendecomposition whose eigenvalue is
        # not exactly zero ("keep"); "drop" removes lambda <= null_cutoff * lambda_max and the known null direction
        ctx.call("pmd_ctx_set_null_cutoff", -1.0 if null_directions == "keep" else float(null_cutoff))
        # host RNG: the seed is the first np.random draw (only when none was given); rank 0's draw counts
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        dist = Dist(distributed)
        seed = dist.broadcast_object(seed)
        own = ownership_plan((d1, d2), block_sizes, dist.world, dist.rank)
        K = int(background_rank)
        streamable = _stream_source_problem(dataset_obj, distributed) is None
        free_bytes = _device_free_bytes(ctx.device) if (stream is None and streamable) else 0
        streamed = _plan_mode(stream, T, d1 * d2, free_bytes, streamable) == "stream"

        movie, stats, frames, frame_range, window_chunks = _load_statistics_background(
            ctx, dist, own, dataset_obj, streamed, (frame_range, window_chunks, max_components, temporal_avg_factor, block_sizes),
            K, seed, compute_normalizer, (frame_batch_size, num_workers, tile_batch_bytes), lap)
        geom = _geometry((d1, d2), block_sizes, order)

        display("Running Simulations, block dimensions are {} x {} x {} ".format(geom.b1, geom.b2, window_chunks))
        t0 = time.perf_counter()
        # streams: enqueued on the side stream before the standardise / filter passes, joined by the tile stage
        sim = _ThresholdSim(ctx, geom, window_chunks, sim_iters, sim_conf, seed, thresholds)
        lap("simulation", t0)

        display("Loading Data")
        std = _standardize_filter(ctx, dist, own, movie, stats, frames, K, single_copy, pixel_weighting, temporal_avg_factor, lap)

        display("Obtaining blocks and running local SVD")
        win = grid.temporal_windows(len(frames), window_chunks, temporal_avg_factor, max_components, display=display)
        tabs = _tile_tables(ctx, geom, spatial_avg_factor)
        tl = _tile_stage(ctx, dist, own, geom, tabs, std, win, sim,
                         (max_consecutive_failures, seed, temporal_denoiser, spatial_denoiser), tile_batch_bytes, lap)
        del tabs
        if streamed:
            std = std._replace(xf=None)   # lifetime: the filtered fit frames are read by the tile stage only (Z comes from pass 2)

        pending_u, cols = _assemble_u(ctx, geom, tl, stats.basis_dev, K, lap)   # the CSR download rides the side stream from here
        tile_ranks_out = cols.ranks.astype(np.int32)
        tl, cols = _virtual_tiles(ctx, dist, tl, cols)

        # ---- orthogonalisation (decomposition.py:860-881)
        display("Performing rank pruning and orthogonalization for fast sparse regression.")
        t0 = time.perf_counter()
        wt = _weight_tiles(ctx, geom, tl, cols)
        rt = _right_matrix(ctx, dist, tl, cols, std.pj_dev, K, win.crop, (rank_prune, rank_prune_factor), seed, orthogonalizer,
                           return_diagnostics)
        zb = _ZBuilder(ctx, dist, own, geom, movie, stats, std, tl, cols, wt.uw_dev, K, lap)
        if rt.use_right:
            rotate = std.all_frames and win.crop == T and not rank_prune and pixel_weighting is None
            mix, t0 = _factored_mixing(ctx, dist, geom, tl, cols, wt, rt, zb, stats.basis_dev, K, T,
                                       (orthogonalizer, null_directions == "keep", rotate), lap, t0)
        else:
            mix = _dense_mixing(ctx, geom, tl, cols, wt, rt, stats.basis_dev, K, std.single_copy)
        rp = mix.rp
        display("After performing rank reduction, the updated rank is {}".format(rp + (1 if mix.null_tail else 0)))
        lap("orthogonalize", t0)

        # ---- V = P^T U^T X over the whole movie (pmd_loader.py:316-346); already enqueued on the Cholesky route
        display("Running sparse regression")
        t0 = time.perf_counter()
        shard = mix.shard and rp <= T
        Z = mix.Z if mix.Z is not None else zb.build(everywhere=True, bg_strip=mix.bg_strip)
        _dbg("Z", Z)
        lap("v_projection", t0)

        # ---- V = P^T Z and the final SVD (decomposition.py:885, :894-904)
        display("Final reformat of data into complete SVD")
        t0 = time.perf_counter()
        if rp <= T:
            display("Short matrix, using leftward SVD routine")
        else:
            display("Tall matrix, using rightward SVD routine")
        Vp = torch.empty((rp, T), dtype=torch.float32, device=ctx.device) if return_diagnostics else None
        extra_row = cols.R - cols.Rc  # the reference's placeholder background column (a zero row of R)
        hosts = outs = None
        null_info = mix.null_info
        if rt.use_right and rp <= T:
            hosts, null_info = _factored_svd(ctx, dist, tl, cols, rt, mix, Z, T, shard, extra_row, Vp)
        else:
            outs, Vp = _dense_svd(ctx, cols, rt, mix, Z, T, Vp)
        ctx.sync()
        lap("final_svd", t0)
        t0 = time.perf_counter()
        u_r = pending_u.finish()      # streams: the CSR download is joined after the final SVD
        root_only = shard and dist.rank != 0   # sharded global stage: the results live on rank 0
        r_mat, s, vt = _host_results(hosts, outs, mix.null_tail, extra_row, root_only)
        lap("d2h_results", t0)
        display("Matrix decomposition completed")

        mean_img, std_img = _statistic_images(ctx, dist, own, geom, stats)
        final_movie = None if root_only else PMDArray(u_r, r_mat, s, vt, (T, d1, d2), order, mean_img, std_img)
        lap.timings["total"] = time.perf_counter() - t_start
        if not return_diagnostics:
            return final_movie
        diag = {
            "seed": seed, "frames": list(frames), "thresholds": (float(tl.thresholds[0]), float(tl.thresholds[1])),
            "sim_stats": tl.sim_stats, "tile_ranks": tile_ranks_out, "tile_stats": tl.stats_dev.cpu().numpy(),
            "tile_good": tl.good_dev.cpu().numpy(), "tile_keep": tl.keep_dev.cpu().numpy(), "tile_lambda": tl.lam_dev.cpu().numpy(),
            "tile_ut": tl.ut_dev.cpu().numpy().reshape(len(tile_ranks_out), tl.rpad, tl.ut_dev.shape[2]),
            "origins": tl.origins[::tl.nvt], "pix": tl.pix_c[::tl.nvt], "block_weights": geom.block_weights,
            "max_components": tl.r, "rank_before": cols.R, "rank_after": rp + (1 if mix.null_tail else 0), "timings": lap.timings,
            "orthogonalizer": ("cholesky" if (rt.use_right and mix.chol_ok) else "eigh"),
            "crop": win.crop, "dpad": tl.ut_dev.shape[2], "v_proj": Vp.cpu().numpy(), "eig_order": min(rp, T),
            "col_sigma": rt.col_sigma, "n_tile_cols": cols.Rt,
            "null_direction": dict(null_info, split_off=bool(mix.null_tail)),
            "streamed": bool(streamed), "stream_bytes_uploaded": int(movie.bytes_uploaded),
        }
        return final_movie, diag
    finally:
        _release(ctx, own_ctx)
