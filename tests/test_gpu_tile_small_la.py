"""
The other kernels of the 64-row tile stage, entry point by entry point (GPU): pmdk_small_qr, pmdk_small_eig and
pmdk_roughness of csrc/small_la.hip and pmdk_tile_pool_bin of csrc/prep.hip, against float64.  tests/small_la_ref.py
holds the inputs, the references, the restatements, the bounds and their derivations; tests/test_small_la_ref.py shows,
without a GPU, that the inputs have the ranks, condition numbers and spectra relied on here and that the bounds are sharp
and reject mutated references.

Every case runs a handful of tiles plus one guard tile.  Whatever a kernel writes is pre-filled with a NaN of a payload no
arithmetic produces, so "not written" is checked to the bit; whatever the contract (include/pmd_hip.h) says is not read
holds NaN; every input is compared with its host copy, bit for bit, after the calls.  The leading n x n block of an
eigenproblem must be finite by contract, so no NaN or Inf is ever fed into it.
"""
import numpy as np
import pytest

from tests import small_la_ref as R
from tests.tile_gemm_ref import round_up, time_ld
from tests.util import context_under

pytestmark = pytest.mark.gpu

PRE32 = 0x7FC12345
PRE64 = 0x7FF8000012345678

# largest observed figure / bound (or, for the fp32-storage QR, / FACTOR x the restatement's figure); printed by the last test
WORST = {}


def note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


def _t():
    import torch

    return torch


def P(t):
    from localmd_amd._lib import ptr

    return ptr(t)


def dev(ctx, a):
    return _t().from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def prefilled(ctx, shape, double=False):
    torch = _t()
    if double:
        return torch.full(shape, PRE64, dtype=torch.int64, device=ctx.device).view(torch.float64)
    return torch.full(shape, PRE32, dtype=torch.int32, device=ctx.device).view(torch.float32)


def kept(a):
    """where the prefill is still there, to the bit"""
    return a.view(np.int64) == PRE64 if a.dtype == np.float64 else a.view(np.int32) == PRE32


def same_bits(a, b):
    view = np.int64 if a.dtype == np.float64 else np.int32
    return np.array_equal(np.ascontiguousarray(a).view(view), np.ascontiguousarray(b).view(view))


@pytest.fixture(scope="module")
def rocsolver_ctx():
    ctx = context_under({"PMD_SMALL_EIG": "rocsolver"})
    yield ctx
    ctx.close()


# ---- small_qr --------------------------------------------------------------------------------------------------------
class QrBuffers:
    """Yt[tile][comp][q] with y_ld != q_ld and tile strides larger than needed; NaN in every row >= l, every column >= P,
    the gap between the tiles and the guard tile"""

    def __init__(self, P_, l, n):
        self.P, self.l, self.n = P_, l, n
        self.rows_y = max(l, 64)
        self.y_ld, self.q_ld = round_up(P_, 16) + 16, round_up(P_, 4) + 8
        self.y_stride, self.q_stride = self.rows_y * self.y_ld + 48, 64 * self.q_ld + 24

    def host_y(self, tiles, scale=1.0):
        Y = np.full((self.n + 1, self.y_stride), np.nan, dtype=np.float32)
        for b, tile in enumerate(tiles):
            block = np.full((self.rows_y, self.y_ld), np.nan, dtype=np.float32)
            block[:self.l, :self.P] = tile.T * np.float32(scale)
            Y[b, :self.rows_y * self.y_ld] = block.ravel()
        return Y

    def call(self, ctx, y_d, q_d):
        return ctx.lib.pmdk_small_qr(ctx.handle, P(y_d), self.y_stride, self.y_ld, self.P, self.l, P(q_d), self.q_stride, self.q_ld,
                                     self.n)

    def q_of(self, got, b):
        return got[b, :64 * self.q_ld].reshape(64, self.q_ld)


def qr_run(ctx, buf, tiles, scale=1.0):
    host = buf.host_y(tiles, scale)
    y_d = dev(ctx, host)
    q_d = prefilled(ctx, (buf.n + 1, buf.q_stride))
    assert buf.call(ctx, y_d, q_d) == 0
    ctx.sync()
    assert same_bits(y_d.cpu().numpy(), host), "the input changed"
    return q_d.cpu().numpy()


@pytest.mark.parametrize("P_,l", R.QR_SHAPES)
def test_small_qr(gpu_ctx, P_, l):
    """Two well-conditioned tiles (cond_2 <= 1e3), a graded one, one of rank 5, one with zero trailing columns and a constant
    one, against numpy.linalg.qr of the widened matrix (LAPACK's sign convention, the kernel's: columns agree sign
    included).  fp64 storage: |Q - Q64| <= 2^-24 |Q64| + 64 P 2^-53 cond_2 entrywise on the well-conditioned tiles,
    orthonormality <= min(5e-6, (P + 2) 2^-24) and |Y - Q Q^T Y| <= small_la_ref.qr_proj_bound on every tile (derived in
    small_la_ref).  fp32 storage ((314, 60), (629, 64), (628, 64)): the two caps, and each of the three figures at most
    FACTOR = 4 times that of the NumPy restatement of the kernel on the same tile.  Rows [nref, 64), columns [P, q_ld), the
    gap between the tiles and the guard tile keep their prefill; Y 2^24 and Y 2^-24 give the same bits.

    Measured on MI355X, worst over the shapes, figure / bound.  fp64 storage: distance to Q64 0.995 (the output rounding
    term, which an entry just below a rounding boundary nearly fills), orthonormality 0.139, projection 0.204.  fp32
    storage: all three figures equal those of the restatement to every printed digit on all eighteen tiles, that is 0.25 of
    FACTOR times it (orthonormality 3e-8 .. 6.5e-7, projection 8e-8 .. 3.1e-6, distance 0.95 .. 1.4e-7).  No shape and no
    tile showed a scale dependence."""
    ctx = gpu_ctx
    storage = R.qr_storage(P_, l)
    tiles = R.qr_tiles(P_, l)
    nref = min(P_, l)
    buf = QrBuffers(P_, l, len(tiles))
    got = qr_run(ctx, buf, tiles)
    assert kept(got[buf.n]).all(), "guard tile written"
    for b, Y in enumerate(tiles):
        what = (P_, l, storage, b, R.QR_TILE_KINDS[b])
        block = buf.q_of(got, b)
        assert kept(got[b, 64 * buf.q_ld:]).all(), (what, "gap between the tiles written")
        assert kept(block[nref:]).all(), (what, "rows >= min(P, l) written")
        assert kept(block[:, P_:]).all(), (what, "columns >= P written")
        Q = block[:nref, :P_].T
        assert np.isfinite(Q).all(), what
        well = b in R.QR_WELL
        Q64 = R.qr_reference(Y) if well else None
        orth, proj, dist = R.qr_figures(Q, Y, Q64)
        assert orth <= R.QR_ORTH_CAP and proj <= R.qr_proj_cap(Y), (what, orth, proj)
        if storage == "f64":
            assert orth <= R.qr_orth_bound(P_), (what, orth)
            assert proj <= R.qr_proj_bound(Y), (what, proj, R.qr_proj_bound(Y))
            note("qr f64 orthonormality", orth / R.qr_orth_bound(P_))
            note("qr f64 projection", proj / R.qr_proj_bound(Y))
            if well:
                err, bound = np.abs(Q.astype(np.float64) - Q64), R.qr_dist_bound(Q64, R.qr_cond(Y), P_)
                assert np.all(err <= bound), (what, float((err / bound).max()))
                note("qr f64 distance to Q64", (err / bound).max())
        else:
            o_r, p_r, d_r = R.qr_figures(R.qr_restated(Y, storage), Y, Q64)
            print(f"\nsmall_qr {what}: orthonormality {orth:.3g} (restated {o_r:.3g}), projection {proj:.3g} ({p_r:.3g}), "
                  f"distance {dist} ({d_r})")
            assert orth <= R.FACTOR * o_r, (what, orth, o_r)
            assert proj <= R.FACTOR * p_r, (what, proj, p_r)
            note("qr f32 orthonormality", orth / (R.FACTOR * o_r))
            note("qr f32 projection", proj / (R.FACTOR * p_r))
            if well:
                assert dist <= R.FACTOR * d_r, (what, dist, d_r)
                note("qr f32 distance to Q64", dist / (R.FACTOR * d_r))
    for s in R.SCALES:
        scaled = qr_run(ctx, buf, tiles, s)
        differ = [b for b in range(buf.n) if not same_bits(scaled[b], got[b])]
        assert not differ, (P_, l, storage, s, "Qt depends on the scale of Y in tiles", differ)


@pytest.mark.parametrize("P_,l", R.QR_UNSUPPORTED)
def test_small_qr_unsupported(gpu_ctx, P_, l):
    """One row more than fits the LDS at 64 columns, and 65 columns: PMD_ERR_UNSUPPORTED, nothing written, and the context
    serves the next call."""
    ctx = gpu_ctx
    assert R.qr_storage(P_, l) is None
    rng = np.random.default_rng(P_)
    buf = QrBuffers(P_, l, 3)
    y_d = dev(ctx, buf.host_y([rng.standard_normal((P_, l)).astype(np.float32) for _ in range(3)]))
    q_d = prefilled(ctx, (buf.n + 1, buf.q_stride))
    assert buf.call(ctx, y_d, q_d) == R.PMD_ERR_UNSUPPORTED
    ctx.sync()
    assert kept(q_d.cpu().numpy()).all(), "an unsupported call wrote to Qt"
    tiles = R.qr_tiles(7, 20)
    ok = QrBuffers(7, 20, len(tiles))
    got = qr_run(ctx, ok, tiles)
    Q = ok.q_of(got, 0)[:7, :7].T
    assert R.qr_figures(Q, tiles[0])[0] <= R.qr_orth_bound(7)


# ---- small_eig -------------------------------------------------------------------------------------------------------
_EIG_MATS = {}


def eig_mats(n):
    if n not in _EIG_MATS:
        _EIG_MATS[n] = R.eig_mats(n)
    return _EIG_MATS[n]


def eig_call(ctx, g_d, slices, n, mode, tol, n_t):
    Nout = prefilled(ctx, (n_t + 1, 64, 64), double=True)
    lam = prefilled(ctx, (n_t + 1, 64), double=True)
    ctx.call("pmdk_small_eig", P(g_d), slices, n, mode, tol, P(Nout), P(lam), n_t)
    ctx.sync()
    V, L = Nout.cpu().numpy(), lam.cpu().numpy()
    assert kept(V[n_t]).all() and kept(L[n_t]).all(), "guard tile written"
    outside = np.ones((64, 64), dtype=bool)
    outside[:n, :n] = False
    assert np.all(V[:n_t][:, outside] == 0), "entries outside n x n must be exact zeros"
    assert np.all(L[:n_t, n:] == 0), "eigenvalues beyond the order must be exact zeros"
    assert np.isfinite(V[:n_t]).all() and np.isfinite(L[:n_t]).all()
    return V[:n_t, :n, :n], L[:n_t, :n]


def check_mode0(route, what, M, w, V, L):
    """the bounds of _check_eig (test_gpu_tile_kernels_wide.py), lambda_max read as max |lambda|"""
    n = M.shape[0]
    amax = float(np.abs(w).max())
    assert np.all(np.diff(L) <= 1e-9 * amax), (what, "not descending")
    err = np.abs(L - w)
    tol = 1e-9 * np.abs(w) + 1e-12 * amax
    assert np.all(err <= tol), (what, "eigenvalues", float((err / np.maximum(tol, 1e-300)).max()))
    orth = np.abs(V.T @ V - np.eye(n)).max()
    resid = np.abs(M @ V - V * L[None, :]).max()
    assert orth < 1e-12, (what, "orthonormality", float(orth))
    assert resid <= 1e-11 * amax, (what, "residual", float(resid / amax))
    if amax > 0:
        note(f"eig {route} eigenvalue", (err / tol).max())
        note(f"eig {route} residual", resid / (1e-11 * amax))
    note(f"eig {route} orthonormality", orth / 1e-12)


def check_null_modes(route, what, M, w, V0, L0, mode, tol, N, L):
    n = M.shape[0]
    amax = float(np.abs(w).max())
    if route == "ql":
        assert same_bits(L, L0), (what, "eigenvalues differ between the modes")
    else:
        assert np.all(np.abs(L - w) <= 1e-9 * np.abs(w) + 1e-12 * amax), (what, "eigenvalues")
    keep = R.eig_keep_rule(L, tol)
    zero_col = ~N.any(axis=0)
    assert np.array_equal(zero_col, ~keep), (what, "zeroed columns are not those with lambda <= tol lambda_max or <= 0",
                                             np.nonzero(zero_col)[0].tolist(), np.nonzero(~keep)[0].tolist())
    keep_ref, pinned = R.eig_expected_keep(w, tol)
    assert np.array_equal(keep[pinned], keep_ref[pinned]), (what, "classification differs from the reference's")
    if not keep.any():
        return
    k = np.nonzero(keep)[0]
    if mode == 2:
        if route == "ql":
            assert same_bits(N[:, k], V0[:, k]), (what, "kept columns differ from those of mode 0")
        else:
            Vk = N[:, k]
            assert np.abs(Vk.T @ Vk - np.eye(k.size)).max() < 1e-12, what
            assert np.abs(M @ Vk - Vk * L[None, k]).max() <= 1e-11 * amax, what
        return
    if route == "ql":
        target = V0[:, k].astype(np.longdouble) / np.sqrt(L[k].astype(np.longdouble))[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(target == 0, np.where(N[:, k] == 0, 0.0, np.inf), np.abs(N[:, k] - target) / np.abs(target)).astype(np.float64)
        assert np.all(rel <= 4 * R.U64), (what, "column / sqrt(lambda)", float(rel.max() / R.U64))
        note("eig ql mode 1 scaling / 4 u", rel.max() / (4 * R.U64))
    W = N[:, k].T @ M @ N[:, k]
    bound = n * 1.1e-11 * amax / np.sqrt(np.outer(L[k], L[k]))
    err = np.abs(W - np.eye(k.size))
    assert np.all(err <= bound), (what, "whitening", float((err / bound).max()))
    note(f"eig {route} whitening", (err / bound).max())


@pytest.mark.parametrize("n", R.EIG_ORDERS)
@pytest.mark.parametrize("route", ["ql", "rocsolver"])
def test_small_eig(gpu_ctx, rocsolver_ctx, route, n):
    """pmdk_small_eig on the default route (small_eig_ql_kernel) and under PMD_SMALL_EIG=rocsolver, same bounds: one launch
    of sixteen different problems (the thirteen kinds of eig_ref.make_sym - diagonal and tridiagonal input take the
    sigma == 0 shortcut - and the project's family of rows over four decades with min(5, n - 1) null directions), in one,
    two and four slices that hold unequal shares plus antisymmetric parts, at scales 1, 2^80 and 2^-80.
    Mode 0: eigenvalues descending and equal to numpy.linalg.eigvalsh to rtol 1e-9 / atol 1e-12 max|lambda|, V^T V = I to
    1e-12, |M V - V diag(lambda)| <= 1e-11 max|lambda|, exact zeros outside n x n and in lam_out from n on.
    Modes 1 and 2, tol 0 and 1e-10: the zeroed columns are exactly those whose returned eigenvalue is <= tol lambda_max or
    <= 0, and that is the reference's classification wherever the mode-0 bound leaves no choice; kept columns of mode 2
    are those of mode 0 bit for bit, those of mode 1 the mode-0 column / sqrt(lambda) to 4 2^-53 (QL route, by its
    epilogue; the rocSOLVER route solves again, so there the kept columns are held to the mode-0 bounds instead), and
    |N^T M N - I|_ij <= n 1.1e-11 max|lambda| / sqrt(lambda_i lambda_j) on the kept ones.
    Outside the leading block the slices hold NaN (QL) or zero (rocSOLVER route, as test_small_eig_through_rocsolver).

    Measured on MI355X, worst over orders, slices, scales and kinds, figure / bound, QL / rocSOLVER: eigenvalues 6.6e-4 /
    1.3e-4, orthonormality 6.4e-3 / 4.0e-2, residual 3.9e-4 / 1.6e-3, whitening 3.4e-5 / 2.0e-5; QL mode-1 scaling 0.59 of
    4 2^-53."""
    ctx = gpu_ctx if route == "ql" else rocsolver_ctx
    mats = eig_mats(n)
    n_t = len(mats)
    for slices in R.EIG_SLICES:
        G1 = R.eig_slices(mats, slices, np.nan if route == "ql" else 0.0, seed=n)
        for scale in R.EIG_SCALES:
            G = G1 * scale
            Ms = R.eig_matrix_of(G, n)
            assert np.isfinite(Ms).all()
            ws = [np.linalg.eigvalsh(Ms[b])[::-1] for b in range(n_t)]
            g_d = dev(ctx, G)
            V0, L0 = eig_call(ctx, g_d, slices, n, 0, 0.0, n_t)
            for b in range(n_t):
                check_mode0(route, (route, n, slices, scale, R.EIG_KINDS[b], "mode 0"), Ms[b], ws[b], V0[b], L0[b])
            for mode in (1, 2):
                for tol in R.EIG_TOLS:
                    N, L = eig_call(ctx, g_d, slices, n, mode, tol, n_t)
                    for b in range(n_t):
                        check_null_modes(route, (route, n, slices, scale, R.EIG_KINDS[b], "mode", mode, "tol", tol), Ms[b], ws[b],
                                         V0[b], L0[b], mode, tol, N[b], L[b])
            assert same_bits(g_d.cpu().numpy(), G), "the input changed"


# ---- tile_pool_bin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.POOL_CASES, ids=lambda c: c.name)
def test_tile_pool_bin(gpu_ctx, case):
    """Full and partial windows (pool_q with -1 pads), pool 1, a = 1, 4 (T no multiple of a: the trailing frames hold NaN),
    10, 2100 bins (above the 8 x 256 threads of a row), 32768 + 70 pixel rows and 32768 + 3 tiles (second launch chunks),
    tile_stride > P ld_ab.  Against float64 means: |xbar - ref| <= (a + 1) 2^-24 mean|x| in every row,
    |abar - ref| <= (a + cnt + 2) 2^-24 (window mean of the bin means of |x|) (small_la_ref.pool_bounds); the case of small
    integers with a and every window count a power of two bit for bit.  Columns from nbins on, the gap between the tiles,
    the guard tile and the rows of xbar from n_rows on keep their prefill.

    Measured on MI355X, worst error / bound over the cases: xbar 0.40, abar 0.38; the exact case exact."""
    ctx = gpu_ctx
    inp = R.pool_inputs(case)
    X, pix, pool_q, Pn, nbins, a = inp["X"], inp["pix"], inp["pool_q"], inp["P"], inp["nbins"], case.a
    n_rows, n_tiles, d = X.shape[0], pix.shape[0], pix.shape[1]
    assert 0 <= pix.min() and pix.max() < n_rows and pool_q.max() < d
    ldx, ld_ab = time_ld(case.T), time_ld(nbins)
    tile_stride = Pn * ld_ab + case.extra
    hx = np.full((n_rows, ldx), np.nan, dtype=np.float32)
    hx[:, :a * nbins] = X[:, :a * nbins]
    x_d, pix_d, pq_d = dev(ctx, hx), dev(ctx, pix), dev(ctx, pool_q)
    xbar_d = prefilled(ctx, (n_rows + 2, ld_ab))
    abar_d = prefilled(ctx, (n_tiles + 1, tile_stride))
    ctx.call("pmdk_tile_pool_bin", P(x_d), ldx, n_rows, P(pix_d), n_tiles, d, P(pq_d), pool_q.shape[1], Pn, a, nbins, P(xbar_d),
             P(abar_d), ld_ab, tile_stride)
    ctx.sync()
    xbar, abar = xbar_d.cpu().numpy(), abar_d.cpu().numpy()
    assert same_bits(x_d.cpu().numpy(), hx) and np.array_equal(pix_d.cpu().numpy(), pix) and np.array_equal(pq_d.cpu().numpy(), pool_q)
    assert kept(xbar[n_rows:]).all(), "rows of xbar from n_rows on written"
    assert kept(xbar[:, nbins:]).all(), "columns of xbar from nbins on written"
    assert kept(abar[n_tiles]).all(), "guard tile written"
    assert kept(abar[:, Pn * ld_ab:]).all(), "gap between the tiles written"
    blocks = abar[:n_tiles, :Pn * ld_ab].reshape(n_tiles, Pn, ld_ab)
    assert kept(blocks[:, :, nbins:]).all(), "columns of abar from nbins on written"
    rx, rxabs, ra, raabs, cnt = R.pool_reference(X, pix, pool_q, a, nbins)
    gx, ga = xbar[:n_rows, :nbins].astype(np.float64), blocks[:, :, :nbins].astype(np.float64)
    assert np.isfinite(gx).all() and np.isfinite(ga).all()
    if R.pool_is_exact(case, pool_q):
        assert np.array_equal(gx, rx) and np.array_equal(ga, ra), "the exact case must be right to the bit"
        return
    bx, ba = R.pool_bounds(a, rxabs, raabs, cnt)
    ex, ea = np.abs(gx - rx), np.abs(ga - ra)
    assert np.all(ex <= bx), (case.name, "xbar", np.argwhere(ex > bx)[:4].tolist(), float((ex / np.maximum(bx, 1e-300)).max()))
    assert np.all(ea <= ba), (case.name, "abar", np.argwhere(ea > ba)[:4].tolist(), float((ea / np.maximum(ba, 1e-300)).max()))
    note("pool_bin xbar", (ex[bx > 0] / bx[bx > 0]).max())
    note("pool_bin abar", (ea[ba > 0] / ba[ba > 0]).max())


# ---- roughness -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ROUGH_CASES, ids=lambda c: "%dx%d_T%d_r%d" % c)
def test_roughness(gpu_ctx, case):
    """Smooth, white, single-pixel / single-frame and all-zero rows (both statistics of a zero row are NaN, 0 / 0, as in the
    reference) against the float64 formulas of evaluation.py:84-126, each within the running error bound of the kernel's
    fp32 arithmetic (small_la_ref.spatial_stat / temporal_stat; below 1e-5 relative, shown on the host).  NaN in Ut from d
    on, in V from T on, in the rows from r on and in the guard tile; rows r..63 of stats and the guard tile keep their
    prefill; with Ut == NULL or V == NULL only the other statistic is written.

    Measured on MI355X, worst error / bound over the cases: spatial 0.19, temporal 0.48."""
    ctx = gpu_ctx
    b1, b2, T, r = case
    d, n = b1 * b2, R.ROUGH_TILES
    U, V = R.rough_inputs(case)
    ref, bound = R.rough_reference(case, U, V)
    u_ld, v_ld = R.rough_u_ld(d), R.rough_v_ld(T)
    hu = np.full((n + 1, 64, u_ld), np.nan, dtype=np.float32)
    hv = np.full((n + 1, 64, v_ld), np.nan, dtype=np.float32)
    hu[:n, :r, :d] = U
    hv[:n, :r, :T] = V
    u_d, v_d = dev(ctx, hu), dev(ctx, hv)
    for which in ("both", "spatial", "temporal"):
        stats = prefilled(ctx, (n + 1, 64, 2))
        ctx.call("pmdk_roughness", P(u_d if which != "temporal" else None), 64 * u_ld, u_ld, b1, b2,
                 P(v_d if which != "spatial" else None), 64 * v_ld, v_ld, T, r, P(stats), n)
        ctx.sync()
        got = stats.cpu().numpy()
        assert kept(got[n]).all(), "guard tile written"
        assert kept(got[:n, r:]).all(), "rows from r on written"
        for k, name in enumerate(("spatial", "temporal")):
            g = got[:n, :r, k]
            if which not in ("both", name):
                assert kept(g).all(), (case, which, name, "written without its input")
                continue
            g = g.astype(np.float64)
            nan = np.isnan(ref[:, :, k])
            assert np.array_equal(np.isnan(g), nan), (case, which, name, "NaN exactly on the all-zero rows")
            err = np.abs(g - ref[:, :, k])[~nan]
            bnd = bound[:, :, k][~nan]
            assert np.all(err <= bnd), (case, which, name, float((err / bnd).max()), np.argwhere(np.abs(g - ref[:, :, k]) > bound[:, :, k])[:4].tolist())
            note(f"roughness {name}", (err / bnd).max())
    assert same_bits(u_d.cpu().numpy(), hu) and same_bits(v_d.cpu().numpy(), hv), "an input changed"


def test_zz_report_worst_ratios():
    """For information: the largest figure / bound each family showed (pytest -s prints it).  Measured on MI355X:
    qr f64 distance 0.995, orthonormality 0.139, projection 0.204; qr f32 (of FACTOR x restatement) 0.25 each;
    eig ql eigenvalue 6.6e-4, orthonormality 6.4e-3, residual 3.9e-4, whitening 3.4e-5, mode-1 scaling 0.59;
    eig rocsolver eigenvalue 1.3e-4, orthonormality 4.0e-2, residual 1.6e-3, whitening 2.0e-5;
    pool_bin xbar 0.40, abar 0.38; roughness spatial 0.19, temporal 0.48."""
    print("\nlargest observed figure / bound:")
    for key in sorted(WORST):
        print(f"  {key:34s} {WORST[key]:.3g}")
    assert all(v <= 1.0 for v in WORST.values())
