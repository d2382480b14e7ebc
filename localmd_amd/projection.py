"""
Projection of frames and new movies onto a stored decomposition's spatial basis.

``project_frames(pmd, frames)`` computes ``C = (U R)^T ((Y - mean_img) / std_img)`` for ``n`` frames ``(n, d1, d2)``
with the decomposition's own standardisation and pixel order; for the movie the decomposition was fitted on,
``C = diag(s) Vt`` in exact arithmetic (the reference forms v = P^T U^T Y_std, r = P W and s Vt = W^T v,
decomposition.py:885-901).  ``project_movie(pmd, movie)`` turns C into a new PMDArray for ``movie`` through the projected
SVD (decomposition.py:885-908).  The reference has the operation only inside its pipeline (``PMDLoader.v_projection``,
pmd_loader.py:316-346, :393-414).

Hot path: ``pmd_group_project`` (csrc/project.hip) reads every frame batch in its source dtype, standardises it while
staging it into LDS and contracts it with the columns of U, grouped by the tables built here; ``C = R^T Z`` then goes
through ``pmd_gemm``.

Group tables (pure NumPy): the columns of U are cut into groups, runs of consecutive columns with at most 64 columns
whose union support is at most P_MAX pixels, where a column joins the open group only if at least 3/4 of its pixels are
already in it.  For a decomposition this gives one group per tile (a tile's columns share the tile rectangle up to
dropped exact zeros; neighbouring tiles share at most half of it), also where two small tiles would fit under P_MAX
together.  Columns with more than P_MAX pixels are wide (the K background columns): runs of at most 64 of them form a
wide set whose union support is cut into P_MAX-pixel chunks, one group per chunk, writing partial sums that the kernel
call reduces in chunk order.
"""
import numpy as np
import scipy.sparse

from ._movie import _device_free_bytes
from ._stream import ToHost, device_context, mean_std, read_batches, upload_f32
from .decomposition import _projected_svd_dev, display
from .pmdarray import PMDArray

# Largest group support: the largest tile the decomposition accepts (40 x 40 pixels, pmd_pick_dvariant), so a tile is
# never split.  The kernel streams a group's pixels through LDS in 64-pixel chunks (34.8 KiB per workgroup, four
# workgroups per CU within the 160 KiB), so LDS bounds the chunk, not the group.
P_MAX = 1600
MAX_ROWS = 64          # columns per group (rows of one A_g: four 16-row MFMA tiles)
ROW_PAD = 16           # A_g rows are padded to whole MFMA row tiles ...
PIX_PAD = 64           # ... and its pixel count to whole LDS chunks
GROUP_FIELDS = 6       # {pix_off, p_g, a_off, out_row, r_g, to_ws}


def _pad(x, m):
    return (x + m - 1) // m * m


def group_tables(u, fov, order):
    """Group tables of the sparse (D x R) spatial basis ``u`` of a decomposition with FOV ``fov`` = (d1, d2) and pixel
    order ``order``.  Returns a dict of NumPy arrays:

    groups   int64 (G, 6)  {pix_off, p_g, a_off, out_row, r_g, to_ws} per group
    pix      int32         C-order pixel ids c = i d2 + j of all groups, sorted within a group
    a        float32       the blocks A_g, round_up(r_g, 16) x round_up(p_g, 64), row-major, zero padded
    wide     int64 (W, 4)  {z_row, ws_row0, parts, stride} per wide column
    col0     int64 (G,)    first column of U that a group's rows hold
    n_cols, n_partial_rows, D
    """
    d1, d2 = (int(x) for x in fov)
    D = d1 * d2
    csc = scipy.sparse.csc_matrix(u)
    if csc.shape[0] != D:
        raise ValueError("U has {} rows, the field of view {} x {} has {} pixels".format(csc.shape[0], d1, d2, D))
    n_cols = int(csc.shape[1])
    # U row id (pixel in `order`) -> C-order pixel id
    c_of_u = np.empty(D, dtype=np.int64)
    c_of_u[np.arange(D).reshape((d1, d2), order=order).reshape(-1)] = np.arange(D)
    indptr = csc.indptr.astype(np.int64)
    cols_c = [None] * n_cols
    cols_v = [None] * n_cols
    for j in range(n_cols):
        c = c_of_u[csc.indices[indptr[j]:indptr[j + 1]]]
        srt = np.argsort(c, kind="stable")
        cols_c[j] = c[srt]
        cols_v[j] = csc.data[indptr[j]:indptr[j + 1]][srt]
    nnz = np.diff(indptr)

    groups, pix_parts, a_parts, wide, col0 = [], [], [], [], []
    n_pix = n_a = n_ws = 0

    def add_group(pixels, dense, out_row, to_ws, first_col):
        nonlocal n_pix, n_a
        r, p = dense.shape
        blk = np.zeros((_pad(r, ROW_PAD), _pad(p, PIX_PAD)), dtype=np.float32)
        blk[:r, :p] = dense
        groups.append((n_pix, p, n_a, out_row, r, to_ws))
        col0.append(first_col)
        pix_parts.append(pixels.astype(np.int32))
        a_parts.append(blk.reshape(-1))
        n_pix += p
        n_a += blk.size

    mark = np.zeros(D, dtype=bool)
    j = 0
    while j < n_cols:
        if nnz[j] > P_MAX:
            j1 = j
            while j1 < n_cols and j1 - j < MAX_ROWS and nnz[j1] > P_MAX:
                j1 += 1
            r = j1 - j
            pixels = np.unique(np.concatenate(cols_c[j:j1]))
            dense = np.zeros((r, len(pixels)))
            for k in range(r):
                dense[k, np.searchsorted(pixels, cols_c[j + k])] = cols_v[j + k]
            parts = -(-len(pixels) // P_MAX)
            for ch in range(parts):
                sl = slice(ch * P_MAX, (ch + 1) * P_MAX)
                add_group(pixels[sl], dense[:, sl], n_ws + ch * r, 1, j)
            wide += [(j + k, n_ws + k, parts, r) for k in range(r)]
            n_ws += parts * r
            j = j1
            continue
        members = [cols_c[j]]
        mark[cols_c[j]] = True
        size = len(cols_c[j])
        j1 = j + 1
        while j1 < n_cols and j1 - j < MAX_ROWS and nnz[j1] <= P_MAX:
            c = cols_c[j1]
            inside = mark[c]
            new = c[~inside]
            if 4 * (len(c) - len(new)) < 3 * len(c) or size + len(new) > P_MAX:
                break
            mark[new] = True
            members.append(new)
            size += len(new)
            j1 += 1
        pixels = np.sort(np.concatenate(members))
        mark[pixels] = False
        dense = np.zeros((j1 - j, len(pixels)))
        for k in range(j1 - j):
            dense[k, np.searchsorted(pixels, cols_c[j + k])] = cols_v[j + k]
        add_group(pixels, dense, j, 0, j)
        j = j1

    tabs = {
        "groups": np.array(groups, dtype=np.int64).reshape(-1, GROUP_FIELDS),
        "pix": np.concatenate(pix_parts) if pix_parts else np.zeros(0, np.int32),
        "a": np.concatenate(a_parts) if a_parts else np.zeros(0, np.float32),
        "wide": np.array(wide, dtype=np.int64).reshape(-1, 4),
        "col0": np.array(col0, dtype=np.int64),
        "n_cols": n_cols, "n_partial_rows": int(n_ws), "D": D,
    }
    validate_tables(tabs)
    return tabs


def validate_tables(t):
    """Raise ValueError unless every index the kernel follows stays inside its array (the kernel trusts the tables)."""
    g, pix, a, wide = t["groups"], t["pix"], t["a"], t["wide"]
    D, n_cols, n_ws = int(t["D"]), int(t["n_cols"]), int(t["n_partial_rows"])
    if g.ndim != 2 or g.shape[1] != GROUP_FIELDS or wide.ndim != 2 or wide.shape[1] != 4:
        raise ValueError("group tables: bad table shapes")
    if pix.size and (int(pix.min()) < 0 or int(pix.max()) >= D):
        raise ValueError("group tables: pixel id outside [0, {})".format(D))
    if not len(g):
        return
    pix_off, p, a_off, out_row, r, to_ws = (g[:, k] for k in range(GROUP_FIELDS))
    if np.any(p < 0) or np.any(p > P_MAX) or np.any(r < 1) or np.any(r > MAX_ROWS) or not np.all((to_ws == 0) | (to_ws == 1)):
        raise ValueError("group tables: a group has more than {} pixels or a row count outside [1, {}]".format(P_MAX, MAX_ROWS))
    if pix_off[0] != 0 or np.any(pix_off[1:] != pix_off[:-1] + p[:-1]) or pix_off[-1] + p[-1] != pix.size:
        raise ValueError("group tables: pixel offsets are not monotone / do not cover the pixel list")
    a_len = _pad(r, ROW_PAD) * _pad(p, PIX_PAD)
    if a_off[0] != 0 or np.any(a_off[1:] != a_off[:-1] + a_len[:-1]) or a_off[-1] + a_len[-1] != a.size:
        raise ValueError("group tables: A offsets are not monotone / do not cover the value array")
    limit = np.where(to_ws == 1, n_ws, n_cols)
    if np.any(out_row < 0) or np.any(out_row + r > limit):
        raise ValueError("group tables: output rows outside Z / the partial-sum workspace")
    if len(wide):
        z_row, row0, parts, stride = (wide[:, k] for k in range(4))
        if (np.any(z_row < 0) or np.any(z_row >= n_cols) or np.any(row0 < 0) or np.any(parts < 1) or np.any(stride < 1)
                or np.any(row0 + (parts - 1) * stride >= n_ws)):
            raise ValueError("group tables: wide rows outside Z / the partial-sum workspace")
    elif n_ws:
        raise ValueError("group tables: partial rows without wide rows")


def tables_for(pmd):
    """The group tables of a PMDArray, built on first use and cached on it (like its combined temporal matrix)."""
    tabs = getattr(pmd, "_groups", None)
    if tabs is None:
        tabs = group_tables(pmd.u, pmd.shape[1:], pmd.order)
        pmd._groups = tabs
    return tabs


# ---- device side ---------------------------------------------------------------------------------------------------
class DeviceTables:
    """The group tables on the device, ready for pmd_group_project."""

    def __init__(self, ctx, tabs):
        import torch

        dev = ctx.device
        self.tabs = tabs
        self.n_groups = len(tabs["groups"])
        self.groups = torch.from_numpy(np.ascontiguousarray(tabs["groups"])).to(dev)
        self.pix = torch.from_numpy(np.ascontiguousarray(tabs["pix"] if tabs["pix"].size else np.zeros(1, np.int32))).to(dev)
        self.a = torch.from_numpy(np.ascontiguousarray(tabs["a"] if tabs["a"].size else np.zeros(1, np.float32))).to(dev)
        self.wide = torch.from_numpy(np.ascontiguousarray(tabs["wide"] if len(tabs["wide"]) else np.zeros((1, 4), np.int64))).to(dev)
        self.n_wide = len(tabs["wide"])
        self.n_partial_rows = int(tabs["n_partial_rows"])
        self.n_cols = int(tabs["n_cols"])
        self.D = int(tabs["D"])

    def workspace_bytes(self, ctx, n):
        return int(ctx.lib.pmd_group_project_workspace_bytes(self.n_partial_rows, int(n)))

    def project(self, ctx, batch, elem, n, mean, std, Z, ldz, ws):
        """Z[:n_cols, :n] = grouped U^T of the standardised frames-first batch (n x D, element type elem)."""
        from ._lib import ptr

        ctx.call("pmd_group_project", ptr(batch), int(elem), int(n), self.D, ptr(mean), ptr(std), self.n_groups,
                 ptr(self.groups), ptr(self.pix), ptr(self.a), self.n_partial_rows, self.n_wide, ptr(self.wide), ptr(Z),
                 int(ldz), ptr(ws), 0 if ws is None else ws.numel())


# ---- public surface ------------------------------------------------------------------------------------------------
def _as_frames(pmd, frames):
    """(source with a (n, d1, d2) shape, n).  A single (d1, d2) frame counts as n = 1."""
    try:
        import torch
    except ImportError:     # pragma: no cover - torch is a dependency
        torch = None
    shape = tuple(int(x) for x in frames.shape)
    if len(shape) == 2:
        if torch is not None and isinstance(frames, torch.Tensor):
            frames = frames.reshape((1,) + shape)
        elif isinstance(frames, np.ndarray):
            frames = frames.reshape((1,) + shape)
        else:
            raise ValueError("a (d1, d2) frame must be a NumPy array or a torch tensor")
        shape = (1,) + shape
    if len(shape) != 3:
        raise ValueError("frames must be shaped (n, d1, d2) or (d1, d2), got {}".format(shape))
    if shape[1:] != tuple(pmd.shape[1:]):
        raise ValueError("frames have the field of view {} x {}, the decomposition {} x {}".format(
            shape[1], shape[2], pmd.shape[1], pmd.shape[2]))
    return frames, shape[0]


class _Run:
    """One projection on an open context: uploaded tables, R and the statistics; runs the batches of a source."""

    def __init__(self, ctx, pmd):
        self.ctx = ctx
        self.rank = int(pmd.r.shape[1])
        self.tabs = DeviceTables(ctx, tables_for(pmd))
        self.mean, self.std = mean_std(ctx, pmd)
        self.r = upload_f32(ctx, pmd.r)
        if self.r.shape[0] != self.tabs.n_cols:
            raise ValueError("R has {} rows, U has {} columns".format(self.r.shape[0], self.tabs.n_cols))

    def run(self, src, n, frame_batch_size, num_workers, sink):
        """Project every frame batch of src: Z = grouped U^T Y_std (pmd_group_project), then C = R^T Z (pmd_gemm) into
        the columns sink.dst(t0, nb) names; sink.done(t0, nb) after each batch is enqueued."""
        import torch
        from ._lib import ptr

        ctx, tabs = self.ctx, self.tabs
        buf = {"nb": 0}

        def consume(batch, elem, t0, nb):
            if nb > buf["nb"]:      # the first batch is the largest one
                buf["Z"] = torch.empty((tabs.n_cols, nb), dtype=torch.float32, device=ctx.device)
                ws_bytes = tabs.workspace_bytes(ctx, nb)
                buf["ws"] = torch.empty(ws_bytes, dtype=torch.uint8, device=ctx.device) if ws_bytes else None
                buf["nb"] = nb
            Z = buf["Z"]
            tabs.project(ctx, batch, elem, nb, self.mean, self.std, Z, nb, buf["ws"])
            dst, ldc = sink.dst(t0, nb)
            ctx.call("pmd_gemm", 1, 0, self.rank, nb, tabs.n_cols, 1.0, ptr(self.r), self.rank, ptr(Z), nb, 0.0, ptr(dst), ldc)
            sink.done(t0, nb)

        # a device tensor is cut by the raw frame_batch_size (a host source by whole 1024-frame chunks of it)
        step = max(1, int(frame_batch_size))
        read_batches(ctx, src, [(t0, min(n, t0 + step)) for t0 in range(0, n, step)], frame_batch_size, num_workers, consume)
        sink.finish()


class _OnDevice:
    """C for the whole movie in one device array (rank x T) for project_movie."""

    def __init__(self, C):
        self.C = C

    def dst(self, t0, nb):
        return self.C[:, t0:], self.C.shape[1]

    def done(self, t0, nb):
        pass

    def finish(self):
        pass


def project_frames(pmd, frames, *, frame_batch_size=10000, num_workers=0, device=None, ctx=None):
    """C = (U R)^T ((Y - mean_img) / std_img), (rank, n) float32, for frames shaped (n, d1, d2) (or one (d1, d2) frame).

    Sources: NumPy arrays / memmaps, any lazy_data_loader (TiffArray included), CPU or device torch tensors.  Host
    sources are read in frame batches through the pinned staging ring of the streamed decomposition (uint16 / int16
    travel in their own dtype); device tensors are sliced in place.  C goes to the host batch by batch, so the length
    is bound by host memory only.  Reuses the context of ``pmd.to_device()`` when it is active."""
    frames, n = _as_frames(pmd, frames)
    rank = int(pmd.r.shape[1])
    if n == 0 or rank == 0:
        return np.zeros((rank, n), dtype=np.float32)
    with device_context(pmd, device, ctx) as (ctx, _):
        sink = ToHost(ctx, rank, n)
        _Run(ctx, pmd).run(frames, n, frame_batch_size, num_workers, sink)
        ctx.sync()
        return sink.out


def _movie_bytes(ctx, n_cols, rank, T):
    """Device bytes project_movie holds beyond one batch: C and Vt' (rank x T each), R' and the projected SVD's
    workspace."""
    nk = min(rank, T)
    return 4 * (rank * T + nk * T + n_cols * nk + nk) + int(ctx.lib.pmd_projected_svd_workspace_bytes(n_cols, rank, T))


def project_movie(pmd, dataset_obj, *, frame_batch_size=10000, num_workers=0, device=None, ctx=None):
    """A new PMDArray for ``dataset_obj`` on ``pmd``'s spatial basis: the same U, mean and std; R' = R W', s' and Vt'
    from the projected SVD of C = (U R)^T Y_std (decomposition.py:885-908); components with s' == 0 are dropped
    (:901-904).  C (rank x T floats) is kept on the device: when it cannot fit, a ValueError points to project_frames."""
    import torch

    frames, T = _as_frames(pmd, dataset_obj)
    d1, d2 = pmd.shape[1:]
    rank = int(pmd.r.shape[1])
    if T == 0 or rank == 0:
        raise ValueError("project_movie needs at least one frame and one component (got {} frames, rank {})".format(T, rank))
    with device_context(pmd, device, ctx) as (ctx, _):
        n_cols = int(pmd.u.shape[1])
        need = _movie_bytes(ctx, n_cols, rank, T)
        free = _device_free_bytes(ctx.device)
        if need > free:
            raise ValueError("project_movie: the projection of {} frames on {} components needs about {:.1f} GB of device "
                             "memory, {:.1f} GB are free; use PMDArray.project_frames (C batch by batch on the host) "
                             "instead".format(T, rank, need / 1e9, free / 1e9))
        run = _Run(ctx, pmd)
        C = torch.empty((rank, T), dtype=torch.float32, device=ctx.device)
        run.run(frames, T, frame_batch_size, num_workers, _OnDevice(C))
        R_out, s_out, Vt_out = _projected_svd_dev(ctx, run.r, n_cols, rank, C, rank, T, T)
        ctx.sync()
        r_new, s_new, vt_new = R_out.cpu().numpy(), s_out.cpu().numpy(), Vt_out.cpu().numpy()
        good = s_new != 0
        if not np.all(good):
            r_new, s_new, vt_new = r_new[:, good], s_new[good], vt_new[good, :]
        display("Projected {} frames on {} components".format(T, rank))
        return PMDArray(pmd.u, r_new, s_new, vt_new, (T, d1, d2), pmd.order, pmd.mean_img, pmd.var_img)
