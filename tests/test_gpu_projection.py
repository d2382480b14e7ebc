"""Projection of frames and movies onto a stored decomposition's basis on the GPU: the pmd_group_project kernel against
fp64 NumPy, its batch invariance, project_frames / project_movie end to end and across sources."""
import os

import numpy as np
import pytest
import scipy.sparse

import localmd_amd
from localmd_amd import decomposition as Dm
from localmd_amd import projection as P
from localmd_amd._lib import ptr
from localmd_amd.dataset import ArrayDataset
from localmd_amd.synthetic import make_movie

pytestmark = pytest.mark.gpu
Dm.QUIET = True
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_small.npz")
ELEM = {np.float32: 0, np.uint16: 1, np.int16: 2}


# ---- kernel -------------------------------------------------------------------------------------------------------
def _kernel_case(seed=0):
    """A C-order U on a 48 x 50 FOV with one block of r columns on a random p-pixel support for every (r, p) of the
    issue's grid, then three dense columns (2400 > P_MAX pixels: split into two chunks)."""
    rng = np.random.default_rng(seed)
    d1, d2 = 48, 50
    D = d1 * d2
    rows, cols, vals = [], [], []
    j = 0
    for r in (1, 5, 16, 17, 33, 64):
        for p in (1, 7, 400, P.P_MAX):
            sup = np.sort(rng.choice(D, p, replace=False))
            for _ in range(r):
                rows.append(sup)
                cols.append(np.full(p, j))
                vals.append(rng.standard_normal(p))
                j += 1
    for _ in range(3):
        rows.append(np.arange(D))
        cols.append(np.full(D, j))
        vals.append(rng.standard_normal(D) * 0.02)
        j += 1
    u = scipy.sparse.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(D, j))
    return u, (d1, d2)


def _movie(n, D, dtype, rng):
    mean = (1000.0 + rng.uniform(-20, 20, D)).astype(np.float32)
    std = (10.0 * rng.uniform(0.8, 1.2, D)).astype(np.float32)
    y = mean[None, :] + std[None, :] * rng.standard_normal((n, D))
    if dtype != np.float32:
        y = np.rint(y)
    return y.astype(dtype), mean, std


def _run_kernel(ctx, dt, y_dev, elem, n, mean, std, extra_rows=5, ldz=None):
    import torch

    ldz = n + 3 if ldz is None else ldz
    Z = torch.full((dt.n_cols + extra_rows, ldz), float("nan"), dtype=torch.float32, device=ctx.device)
    wb = dt.workspace_bytes(ctx, n)
    ws = torch.empty(max(wb, 1), dtype=torch.uint8, device=ctx.device)
    dt.project(ctx, y_dev, elem, n, mean, std, Z, ldz, ws)
    ctx.sync()
    return Z.cpu().numpy()


@pytest.fixture(scope="module")
def kcase(gpu_ctx):
    u, fov = _kernel_case()
    t = P.group_tables(u, fov, "C")
    assert len(t["wide"]) == 3 and t["n_partial_rows"] == 6
    return u, fov, P.DeviceTables(gpu_ctx, t)


@pytest.mark.parametrize("dtype", [np.float32, np.uint16, np.int16])
@pytest.mark.parametrize("n", [1, 3, 31, 64, 1000])
def test_group_project_against_fp64(gpu_ctx, kcase, dtype, n):
    """Per-row error of Z against fp64 U^T Y_std, relative to the row of |U|^T |Y_std| (the scale of an fp32 fma chain's
    rounding: a row norm alone is ill-conditioned for one frame on a few pixels).  Measured at most 1.6e-7 for up to
    2400-term chains (n = 1 and 3; 6e-8 at n = 1000); bound 1e-6.  Rows outside every group and columns >= n stay NaN."""
    import torch

    u, fov, dt = kcase
    D = fov[0] * fov[1]
    rng = np.random.default_rng(n)
    y, mean, std = _movie(n, D, dtype, rng)
    mean_d, std_d = torch.from_numpy(mean).cuda(), torch.from_numpy(std).cuda()
    y_dev = torch.from_numpy(y.view(np.int16) if dtype == np.uint16 else y).cuda()
    Z = _run_kernel(gpu_ctx, dt, y_dev, ELEM[dtype], n, mean_d, std_d)
    ys = (y.astype(np.float32).astype(np.float64) - mean) / std
    ref = np.asarray(u.T @ ys.T)
    scale = np.asarray(abs(u).T @ np.abs(ys).T)
    nc = dt.n_cols
    assert np.all(np.isnan(Z[nc:])) and np.all(np.isnan(Z[:, n:]))
    got = Z[:nc, :n].astype(np.float64)
    assert np.all(np.isfinite(got))
    err = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(scale, axis=1)
    print(f"group_project {np.dtype(dtype).name} n={n}: max row err {err.max():.2e}")
    assert err.max() < 1e-6, err.max()


def test_group_project_batch_invariance(gpu_ctx, kcase):
    """Z[:, f] is bitwise independent of n and of the batch f arrives in; uint16 gives bitwise its fp32 conversion."""
    import torch

    u, fov, dt = kcase
    D = fov[0] * fov[1]
    rng = np.random.default_rng(11)
    N = 300
    y, mean, std = _movie(N, D, np.uint16, rng)
    mean_d, std_d = torch.from_numpy(mean).cuda(), torch.from_numpy(std).cuda()
    y16 = torch.from_numpy(y.view(np.int16)).cuda()
    y32 = torch.from_numpy(y.astype(np.float32)).cuda()
    full = _run_kernel(gpu_ctx, dt, y16, 1, N, mean_d, std_d)[:dt.n_cols, :N]
    full32 = _run_kernel(gpu_ctx, dt, y32, 0, N, mean_d, std_d)[:dt.n_cols, :N]
    assert np.array_equal(full, full32)
    for a, b in [(0, 1), (5, 70), (63, 64), (100, 299), (17, 300)]:
        part = _run_kernel(gpu_ctx, dt, y16[a:b], 1, b - a, mean_d, std_d)[:dt.n_cols, :b - a]
        assert np.array_equal(part, full[:, a:b]), (a, b)


def test_group_project_rejects_bad_arguments(gpu_ctx, kcase):
    import torch
    from localmd_amd._lib import PMDLibraryError

    u, fov, dt = kcase
    D = fov[0] * fov[1]
    y = torch.zeros((4, D), dtype=torch.float32, device=gpu_ctx.device)
    m = torch.zeros(D, dtype=torch.float32, device=gpu_ctx.device)
    Z = torch.zeros((dt.n_cols, 4), dtype=torch.float32, device=gpu_ctx.device)
    ws = torch.empty(dt.workspace_bytes(gpu_ctx, 4), dtype=torch.uint8, device=gpu_ctx.device)
    args = [ptr(y), 0, 4, D, ptr(m), ptr(m), dt.n_groups, ptr(dt.groups), ptr(dt.pix), ptr(dt.a), dt.n_partial_rows,
            dt.n_wide, ptr(dt.wide), ptr(Z), 4, ptr(ws), ws.numel()]
    for k, bad in [(1, 7), (2, -1), (3, 0), (14, 3), (16, ws.numel() - 1), (6, -2)]:
        a = list(args)
        a[k] = bad
        with pytest.raises(PMDLibraryError):
            gpu_ctx.call("pmd_group_project", *a)


# ---- end to end ---------------------------------------------------------------------------------------------------
def _decompose(ctx, mov, order, blocks=(20, 20), frames=None, max_components=6, background_rank=2, seed=3):
    np.random.seed(1)
    return localmd_amd.localmd_decomposition(mov, blocks, frames or mov.shape[0], max_components=max_components,
                                             background_rank=background_rank, order=order, seed=seed, sim_iters=10,
                                             ctx=ctx)


def _ystd_u(pmd, mov):
    ys = (mov.astype(np.float64) - pmd.mean_img.astype(np.float64)) / pmd.var_img.astype(np.float64)
    return np.stack([f.reshape(-1, order=pmd.order) for f in ys])   # (n, D) in U's row order


def _fp64_c(pmd, mov):
    return (pmd.u @ pmd.r.astype(np.float64)).T @ _ystd_u(pmd, mov).T


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


CASES = {
    "synthetic_F": dict(shape=(500, 40, 44), seed=4, order="F", blocks=(20, 20), K=2, mc=6),
    "synthetic_C": dict(shape=(500, 40, 44), seed=4, order="C", blocks=(20, 20), K=2, mc=6),
    "oracle_small": dict(shape=(400, 30, 36), seed=11, order="F", blocks=(20, 16), K=2, mc=5),
}


@pytest.fixture(scope="module")
def decomps(gpu_ctx):
    out = {}
    for name, c in CASES.items():
        mov = make_movie(*c["shape"], seed=c["seed"])
        out[name] = (mov, _decompose(gpu_ctx, mov, c["order"], c["blocks"], max_components=c["mc"], background_rank=c["K"]))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_project_frames_reproduces_s_vt(gpu_ctx, decomps, name):
    """project_frames(original movie) against diag(s) Vt and against fp64 (U R)^T Y_std, normwise.
    Measured: 2.2e-6 against the fp64 restatement and 2.4e-6 against diag(s) Vt (synthetic 40 x 44, both orders),
    8.5e-7 / 9.4e-7 on the oracle_small configuration; bounds 1e-5 for both."""
    mov, pmd = decomps[name]
    C = pmd.project_frames(mov, ctx=gpu_ctx)
    assert C.shape == (len(pmd.s), mov.shape[0]) and C.dtype == np.float32
    e_svt = _rel(C, pmd.s[:, None].astype(np.float64) * pmd.v)
    e_64 = _rel(C, _fp64_c(pmd, mov))
    print(f"{name}: vs diag(s)Vt {e_svt:.2e}, vs fp64 {e_64:.2e}")
    assert e_64 < 1e-5, e_64
    assert e_svt < 1e-5, e_svt


def test_project_frames_sources_agree(gpu_ctx, decomps, tmp_path):
    """ndarray, memmap, lazy_data_loader, CPU and device tensors; two frame_batch_size values; a save_npz / load_npz round
    trip.  Host sources share the staging path: bitwise equal.  Others: within 1e-6 normwise (measured ~1e-7)."""
    import torch

    mov, pmd = decomps["synthetic_F"]
    movu = np.rint(mov * 20).astype(np.uint16)
    for src_mov in (mov, movu):
        ref = pmd.project_frames(src_mov, ctx=gpu_ctx)
        path = tmp_path / "m.bin"
        mm = np.memmap(path, dtype=src_mov.dtype, mode="w+", shape=src_mov.shape)
        mm[:] = src_mov
        mm.flush()
        mm = np.memmap(path, dtype=src_mov.dtype, mode="r", shape=src_mov.shape)
        assert np.array_equal(pmd.project_frames(mm, ctx=gpu_ctx), ref)
        assert np.array_equal(pmd.project_frames(ArrayDataset(src_mov), ctx=gpu_ctx), ref)
        assert np.array_equal(pmd.project_frames(torch.from_numpy(src_mov.astype(np.float32)), ctx=gpu_ctx), ref)
        dev = torch.from_numpy(src_mov.astype(np.float32)).cuda()
        e = _rel(pmd.project_frames(dev, ctx=gpu_ctx), ref)
        assert e < 1e-6, e
        e = _rel(pmd.project_frames(src_mov, frame_batch_size=100, ctx=gpu_ctx), ref)
        assert e < 1e-6, e
        # a single frame, and a leading slice
        c1 = pmd.project_frames(src_mov[7], ctx=gpu_ctx)
        assert c1.shape == (ref.shape[0], 1) and _rel(c1[:, 0], ref[:, 7]) < 1e-6
    f = tmp_path / "pmd.npz"
    localmd_amd.save_npz(f, pmd)
    back = localmd_amd.load_npz(f)
    assert np.array_equal(back.project_frames(mov, ctx=gpu_ctx), pmd.project_frames(mov, ctx=gpu_ctx))
    # an active to_device() context is reused
    pmd.to_device(ctx=gpu_ctx)
    try:
        assert np.array_equal(pmd.project_frames(mov), pmd.project_frames(mov, ctx=gpu_ctx))
    finally:
        pmd.to_host()


def test_project_frames_longer_than_one_batch(gpu_ctx, decomps):
    """Several staged batches (frame_batch_size rounds down to whole 1024-frame batches): equal to one batch per frame
    range within 1e-6, and to fp64."""
    mov, pmd = decomps["synthetic_C"]
    long = np.concatenate([mov] * 5)            # 2500 frames
    C = pmd.project_frames(long, frame_batch_size=1024, ctx=gpu_ctx)
    C1 = pmd.project_frames(long, frame_batch_size=4096, ctx=gpu_ctx)
    assert _rel(C, C1) < 1e-6
    assert _rel(C, _fp64_c(pmd, long)) < 1e-5


def test_project_movie_second_movie(gpu_ctx, decomps):
    """On another movie: Vt' orthonormal, s' non-increasing, sampled frames match fp64 mean + std (UR)(UR)^T Y_std
    (error relative to the standardised reconstruction's norm; measured at most 2.5e-6, bound 1e-5)."""
    mov, pmd = decomps["synthetic_F"]
    mov2 = make_movie(300, 40, 44, seed=99)
    pmd2 = localmd_amd.project_movie(pmd, mov2, ctx=gpu_ctx)
    assert pmd2.shape == mov2.shape
    vt = pmd2.v.astype(np.float64)
    assert np.abs(vt @ vt.T - np.eye(vt.shape[0])).max() < 1e-4
    assert np.all(np.diff(pmd2.s) <= 0) and np.all(pmd2.s > 0)
    ur = pmd.u @ pmd.r.astype(np.float64)
    ys = _ystd_u(pmd, mov2)
    for t in (0, 17, 299):
        rec = ur @ (ur.T @ ys[t])
        ref = pmd.mean_img.astype(np.float64) + pmd.var_img * rec.reshape((40, 44), order=pmd.order)
        got = pmd2[t].astype(np.float64)
        err = np.linalg.norm(got - ref) / np.linalg.norm(pmd.var_img * rec.reshape((40, 44), order=pmd.order))
        print(f"project_movie second movie frame {t}: {err:.2e}")
        assert err < 1e-5, (t, err)


def test_project_movie_original_movie(gpu_ctx, decomps):
    """pmd2[t] against pmd[t], relative to the frame's deviation from the mean: measured at most 2.7e-6, bound 1e-5."""
    mov, pmd = decomps["oracle_small"]
    pmd2 = localmd_amd.project_movie(pmd, mov, ctx=gpu_ctx)
    for t in (0, 5, 399):
        a, b = pmd2[t].astype(np.float64), pmd[t].astype(np.float64)
        err = np.linalg.norm(a - b) / np.linalg.norm(b - pmd.mean_img)
        print(f"project_movie original movie frame {t}: {err:.2e}")
        assert err < 1e-5, (t, err)


def test_project_movie_too_long_raises(gpu_ctx, decomps, monkeypatch):
    mov, pmd = decomps["synthetic_F"]
    monkeypatch.setattr(P, "_device_free_bytes", lambda device: 1000)
    with pytest.raises(ValueError, match="project_frames"):
        localmd_amd.project_movie(pmd, mov, ctx=gpu_ctx)
