"""
Kernel-level tests (GPU) of the small dense algebra of the tile stage that had no entry point of its own: the
generic-width kernels of csrc/wide.hip (pmdk_wide_gram, pmdk_wide_eig, pmdk_wide_rowmix) and the Cholesky whitening of
the 64-row path (pmdk_small_chol), each against float64 NumPy.  Every output buffer holds NaN before the call, so "not
written" and "written as zero" differ; so does every part of an input that the kernel has no business reading.  The
bounds of the Gram matrix and of the row mix are derived (fp64 accumulation of exact products); those of the
eigensolvers are the ones test_small_eig holds the 64-row kernel to.
"""
import numpy as np
import pytest

from tests import tile_stage_ref as R
from tests.util import context_under

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53
U32 = 2.0 ** -24
N_TILES = 3


def _t():
    import torch

    return torch


def P(t):
    from localmd_amd._lib import ptr

    return ptr(t)


def _dev(ctx, a, dtype=None):
    return _t().from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ctx.device)


def _nan(ctx, shape, dtype):
    torch = _t()
    return torch.full(shape, float("nan"), dtype=dtype, device=ctx.device)


@pytest.fixture(scope="module")
def syevd_ctx():
    ctx = context_under({"PMD_WIDE_EIG": "syevd"})
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def rocsolver_ctx():
    ctx = context_under({"PMD_SMALL_EIG": "rocsolver"})
    yield ctx
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 31, 33, 100, 1234])
@pytest.mark.parametrize("rp", [128, 192])
def test_wide_gram(gpu_ctx, rp, length):
    """pmdk_wide_gram, symmetric and cross form (In2 != In: the result is not symmetric, so swapped block indices show),
    one slice and four, leading dimension pmd_time_ld(len) and a pmd_tile_dpad value, rows scaled over three decades,
    NaN behind column len of both inputs.  Element-wise on the sum over the slices
    |got - ref| <= len 2^-53 (|In| |In2|^T): products of fp32 values are exact in fp64, so this is the bound of a sum of
    len terms (derived, not measured).  A slice without positions (len = 33 in four slices: the last two) is exact zeros."""
    ctx, lib = gpu_ctx, gpu_ctx.lib
    rng = np.random.default_rng(rp * 10000 + length)
    dpad = int(lib.pmd_tile_dpad(max(length, 64)))
    assert dpad >= length
    scale = np.logspace(0, 3, rp)[rng.permutation(rp)].astype(np.float32)
    for ld in (int(lib.pmd_time_ld(length)), dpad):
        a = np.full((N_TILES, rp, ld), np.nan, dtype=np.float32)
        b = np.full((N_TILES, rp, ld), np.nan, dtype=np.float32)
        a[:, :, :length] = rng.standard_normal((N_TILES, rp, length)).astype(np.float32) * scale[None, :, None]
        b[:, :, :length] = rng.standard_normal((N_TILES, rp, length)).astype(np.float32) * scale[None, ::-1, None]
        a64, b64 = a[:, :, :length].astype(np.float64), b[:, :, :length].astype(np.float64)
        ad, bd = _dev(ctx, a), _dev(ctx, b)
        for slices in (1, 4):
            for second, s64 in ((None, a64), (bd, b64)):
                G = _nan(ctx, (N_TILES + 1, slices, rp, rp), _t().float64)
                ctx.call("pmdk_wide_gram", P(ad), rp * ld, ld, length, N_TILES, slices, rp, P(G), P(second))
                ctx.sync()
                got = G.cpu().numpy()
                assert np.isnan(got[N_TILES]).all(), "guard tile written"
                assert not np.isnan(got[:N_TILES]).any(), (rp, length, ld, slices)
                cps = 32 * -(-(-(-length // slices)) // 32)
                for k in range(slices):
                    if k * cps >= length:
                        assert np.all(got[:N_TILES, k] == 0), ("an empty slice is not zero", rp, length, slices, k)
                if length == 33 and slices == 4:
                    assert np.all(got[:N_TILES, 2:] == 0)
                ref = np.einsum("nit,njt->nij", a64, s64)
                bound = length * U64 * np.einsum("nit,njt->nij", np.abs(a64), np.abs(s64))
                err = np.abs(got[:N_TILES].sum(axis=1) - ref)
                assert np.all(err <= bound), (rp, length, ld, slices, second is not None, float((err / bound).max()))


# ---------------------------------------------------------------------------------------------------------------------
def _eig_mats(rng, n, n_t, nnull):
    """Tile 0: flat spectrum; tile 1: rows scaled over four decades and nnull exact null directions; the others: rows
    scaled over four decades (the matrices of test_small_eig)."""
    mats = []
    for b in range(n_t):
        A = rng.standard_normal((n, 300)) * np.logspace(0, -4 if b else 0, n)[:, None]
        if b == 1 and nnull:
            A[n - nnull:] = 0
        mats.append(A @ A.T)
    return mats


def _check_eig(call, ctx, mats, width, n, nnull, outside):
    """The assertions of test_small_eig on an eigensolver entry point: call(G, mode, tol, Nout, lam) with
    G[tile][2][width][width] holding 0.25 M + A and 0.75 M - A, A antisymmetric (the symmetrised sum cancels it)."""
    torch = _t()
    n_t = len(mats)
    G = R.antisymmetric_split(mats, width, np.random.default_rng(n))
    if outside == 0.0:
        G = np.nan_to_num(G, nan=0.0)
    Gd = _dev(ctx, G)
    Nout = _nan(ctx, (n_t + 1, width, width), torch.float64)
    lam = _nan(ctx, (n_t + 1, width), torch.float64)
    call(Gd, 0, 0.0, Nout, lam)
    ctx.sync()
    V, L = Nout.cpu().numpy(), lam.cpu().numpy()
    assert np.isnan(V[n_t]).all() and np.isnan(L[n_t]).all(), "guard tile written"
    figures = dict(lam=0.0, orth=0.0, resid=0.0, white=0.0)
    for b in range(n_t):
        w = np.linalg.eigvalsh(mats[b])[::-1]
        assert np.all(np.diff(L[b, :n]) <= 1e-9 * w[0]), b
        figures["lam"] = max(figures["lam"], float(np.max(np.abs(L[b, :n] - w) / (1e-9 * np.abs(w) + 1e-12 * w[0]))))
        np.testing.assert_allclose(L[b, :n], w, rtol=1e-9, atol=1e-12 * w[0])
        assert np.all(L[b, n:] == 0), "eigenvalues beyond the order"
        Vb = V[b, :n, :n]
        mask = np.ones((width, width), dtype=bool)
        mask[:n, :n] = False
        assert np.all(V[b][mask] == 0), "entries outside n x n"
        figures["orth"] = max(figures["orth"], float(np.abs(Vb.T @ Vb - np.eye(n)).max()))
        figures["resid"] = max(figures["resid"], float(np.abs(mats[b] @ Vb - Vb * L[b, :n][None, :]).max() / w[0]))
        assert np.abs(Vb.T @ Vb - np.eye(n)).max() < 1e-12, b
        assert np.abs(mats[b] @ Vb - Vb * L[b, :n][None, :]).max() < 1e-11 * w[0], b
    # mode 1: scaled columns, null guard
    Nout.fill_(float("nan"))
    lam.fill_(float("nan"))
    call(Gd, 1, 1e-10, Nout, lam)
    ctx.sync()
    V1 = Nout.cpu().numpy()
    for b in range(n_t):
        kept = L[b, :n] > 1e-10 * L[b, 0]
        assert kept.sum() == n - (nnull if b == 1 else 0), (b, int(kept.sum()))
        Nn = V1[b, :n, :n]
        W = Nn.T @ mats[b] @ Nn
        figures["white"] = max(figures["white"], float(np.abs(W[np.ix_(kept, kept)] - np.eye(kept.sum())).max()))
        assert np.abs(W[np.ix_(kept, kept)] - np.eye(kept.sum())).max() < 1e-7, b
        assert np.all(Nn[:, ~kept] == 0), b
        mask = np.ones((width, width), dtype=bool)
        mask[:n, :n] = False
        assert np.all(V1[b][mask] == 0)
    assert np.isnan(V1[n_t]).all()
    return figures


def _wide_eig_call(ctx, rp, n, n_t):
    nbytes = int(ctx.lib.pmdk_wide_eig_workspace_bytes(n, n_t))
    ws = _t().full((nbytes,), 0xFF, dtype=_t().uint8, device=ctx.device)

    def call(Gd, mode, tol, Nout, lam):
        ctx.call("pmdk_wide_eig", P(Gd), 2, rp, n, mode, tol, P(Nout), P(lam), n_t, P(ws), nbytes)

    return call


@pytest.mark.parametrize("route", ["syevj", "syevd"])
@pytest.mark.parametrize("rp,n", [(128, 65), (128, 90), (128, 128), (128, 5), (192, 150), (128, 1)])
def test_wide_eig(gpu_ctx, syevd_ctx, rp, n, route):
    """pmdk_wide_eig on the default context (rocSOLVER's batched Jacobi solver) and under PMD_WIDE_EIG=syevd, held to the
    bounds of test_small_eig: eigenvalues descending and equal to numpy.linalg.eigvalsh to rtol 1e-9 / atol 1e-12
    lam_max, vectors orthonormal to 1e-12, |M V - V diag(lam)| < 1e-11 lam_max, zeros outside n x n and beyond the order;
    mode 1 with tol 1e-10 zeroes exactly the min(5, n - 1) null columns of tile 1 and N^T M N = I to 1e-7 on the kept
    ones.  The two slices hold 0.25 M + A and 0.75 M - A, A antisymmetric; NaN outside the leading n x n block.

    Both rocSOLVER solvers meet every bound at these orders.  Measured on MI355X, worst over the orders, syevj / syevd:
    eigenvalue error 4.1e-5 / 1.1e-5 of its bound, orthonormality 4.0e-14 / 4.2e-15, residual 3.9e-14 / 1.2e-15 lam_max,
    whitening 4.1e-9 / 1.2e-10."""
    ctx = gpu_ctx if route == "syevj" else syevd_ctx
    nnull = min(5, n - 1)
    mats = _eig_mats(np.random.default_rng(100 * rp + n), n, N_TILES, nnull)
    fig = _check_eig(_wide_eig_call(ctx, rp, n, N_TILES), ctx, mats, rp, n, nnull, outside=np.nan)
    print(f"\nwide_eig {route} rp {rp} n {n}: eigenvalue error / bound {fig['lam']:.2e}, orthonormality {fig['orth']:.2e}, "
          f"residual / lam_max {fig['resid']:.2e}, whitening {fig['white']:.2e}")


def test_small_eig_through_rocsolver(rocsolver_ctx):
    """The assertions of test_small_eig (n = 50, seven tiles, five null directions in tile 1) on pmdk_small_eig under
    PMD_SMALL_EIG=rocsolver, which runs wide_eig at rp = 64.  Measured on MI355X: eigenvalue error 1.5e-5 of its bound,
    orthonormality 1.4e-14, residual 1.2e-14 lam_max, whitening 6.0e-11."""
    ctx = rocsolver_ctx
    n, n_t = 50, 7
    mats = _eig_mats(np.random.default_rng(4), n, n_t, 5)

    def call(Gd, mode, tol, Nout, lam):
        ctx.call("pmdk_small_eig", P(Gd), 2, n, mode, tol, P(Nout), P(lam), n_t)

    fig = _check_eig(call, ctx, mats, 64, n, 5, outside=0.0)
    print(f"\nsmall_eig via rocSOLVER: eigenvalue error / bound {fig['lam']:.2e}, orthonormality {fig['orth']:.2e}, "
          f"residual / lam_max {fig['resid']:.2e}, whitening {fig['white']:.2e}")


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 31, 33, 400, 2100])
@pytest.mark.parametrize("rp,n_in,n_out", [(128, 90, 37), (128, 128, 128), (192, 150, 150), (128, 70, 1)])
def test_wide_rowmix(gpu_ctx, rp, n_in, n_out, length):
    """pmdk_wide_rowmix in place and out of place (ld_in != ld_out), per-tile N and one shared N; 2100 > 64 x 32 positions
    is the length at which a workgroup takes a second trip of its position loop.  NaN in the input rows from n_in on, in
    the columns from len on and in N outside n_in x n_out.  |out - ref| <= 2^-24 |ref| + n_in 2^-53 (|N|^T |In|): fp64
    accumulation and one rounding to fp32 (derived); rows [n_out, rp) exactly zero up to len; columns from len on and the
    guard tile keep their NaN."""
    ctx, lib, torch = gpu_ctx, gpu_ctx.lib, _t()
    rng = np.random.default_rng(rp + 1000 * n_in + 7 * length)
    ld_in = int(lib.pmd_time_ld(length))
    ld_other = ld_in + 32
    src = np.full((N_TILES + 1, rp, ld_in), np.nan, dtype=np.float32)
    src[:N_TILES, :n_in, :length] = rng.standard_normal((N_TILES, n_in, length)).astype(np.float32)
    Nm = np.full((N_TILES, rp, rp), np.nan)
    Nm[:, :n_in, :n_out] = rng.standard_normal((N_TILES, n_in, n_out))
    Nd = _dev(ctx, Nm)
    x64 = src[:N_TILES, :n_in, :length].astype(np.float64)
    for in_place in (True, False):
        for shared in (False, True):
            ind = _dev(ctx, src)
            ld_out = ld_in if in_place else ld_other
            out = ind if in_place else _nan(ctx, (N_TILES + 1, rp, ld_out), torch.float32)
            ctx.call("pmdk_wide_rowmix", P(ind), rp * ld_in, ld_in, P(Nd), 0 if shared else rp * rp, rp, n_in, n_out, P(out),
                     rp * ld_out, ld_out, length, N_TILES)
            ctx.sync()
            got = out.cpu().numpy()
            nm = np.broadcast_to(Nm[:1], Nm.shape) if shared else Nm
            ref = np.einsum("npc,npt->nct", nm[:, :n_in, :n_out], x64)
            bound = U32 * np.abs(ref) + n_in * U64 * np.einsum("npc,npt->nct", np.abs(nm[:, :n_in, :n_out]), np.abs(x64))
            err = np.abs(got[:N_TILES, :n_out, :length] - ref)
            assert np.all(err <= bound), (in_place, shared, float((err / bound).max()))
            assert np.all(got[:N_TILES, n_out:, :length] == 0), (in_place, shared)
            assert np.isnan(got[:, :, length:]).all(), ("columns from len on written", in_place, shared)
            assert np.isnan(got[N_TILES]).all(), "guard tile written"
            if not in_place:
                assert np.array_equal(ind.cpu().numpy().view(np.int32), src.view(np.int32)), "input changed"


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slices", [1, 2])
@pytest.mark.parametrize("n", R.CHOL_ORDERS)
def test_small_chol(gpu_ctx, n, slices):
    """pmdk_small_chol on the matrices of tile_stage_ref.chol_inputs (test_tile_stage_ref.py shows that no pivot is near
    tol = 1e-10: live ones above 1e-4 dmax, dead ones below 1e-12 dmax; the tiles are scaled by 1, 2^-60, 2^40 and 2^-70, so
    only a rule relative to dmax classifies them right).  Full-rank tiles (cond(M) <= 1e4): N equals
    inv(cholesky(M)^T) of NumPy float64 to 1e-10 relative (cond eps64 with four decades to spare).  Deficient tiles (row 3
    and the last row combinations of earlier rows, one zero row; order 1: the zero matrix): exactly the dead columns of N
    are zero, N^T M N = I on the others to 1e-10, and N agrees with the restated pivot rule.  Zeros outside n x n; the
    slices hold 0.25 M + A and 0.75 M - A (one slice: M + A), A antisymmetric, NaN outside the leading block."""
    ctx, torch = gpu_ctx, _t()
    mats, dead = R.chol_inputs(n)
    G = R.antisymmetric_split(mats, 64, np.random.default_rng(n))
    if slices == 1:
        G = G.sum(axis=1, keepdims=True)
    n_t = len(mats)
    Gd = _dev(ctx, G)
    Nout = _nan(ctx, (n_t + 1, 64, 64), torch.float64)
    ctx.call("pmdk_small_chol", P(Gd), slices, n, R.CHOL_TOL, P(Nout), n_t)
    ctx.sync()
    got = Nout.cpu().numpy()
    assert np.isnan(got[n_t]).all(), "guard tile written"
    assert not np.isnan(got[:n_t]).any()
    outside = np.ones((64, 64), dtype=bool)
    outside[:n, :n] = False
    for b, M in enumerate(mats):
        Nb = got[b, :n, :n]
        assert np.all(got[b][outside] == 0), (n, b)
        zero_cols = np.nonzero(np.all(Nb == 0, axis=0))[0].tolist()
        assert zero_cols == dead[b], (n, b, zero_cols)
        live = np.ones(n, dtype=bool)
        live[dead[b]] = False
        if not dead[b]:
            ref = np.linalg.inv(np.linalg.cholesky(M).T)
            assert np.abs(Nb - ref).max() <= 1e-10 * np.abs(ref).max(), (n, b, float(np.abs(Nb - ref).max() / np.abs(ref).max()))
        else:
            W = Nb.T @ M @ Nb
            assert np.abs(W[np.ix_(live, live)] - np.eye(int(live.sum()))).max(initial=0.0) < 1e-10, (n, b)
            ref = R.chol_whiten_ref(G[b], n, R.CHOL_TOL)[0]
            assert np.abs(Nb - ref).max() <= 1e-10 * max(np.abs(ref).max(), 1e-300), (n, b)
