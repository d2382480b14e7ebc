"""Demixing on the GPU (localmd_amd.demix, csrc/hals.hip): pmd_hals_sweep through the C ABI bit for bit against its NumPy
emulation, pmd_hals_pixels against float64, and demix end to end against the dense float64 reference of
tests/hals_ref.py on the expanded movie: invariances over residency, pixel order and ROI form, the tie to
extract_traces, a planted pair of overlapping cells, and the growth of device memory with the movie's length."""
import ctypes as C
import importlib

import numpy as np
import pytest
import scipy.sparse

import localmd_amd
from localmd_amd._lib import PMDLibraryError, ptr
from localmd_amd.pmdarray import PMDArray
from localmd_amd.traces import roi_weights
from tests import hals_ref as HR
from tests.consumer_fuzz import REF32, rel as _rel        # REF32: the fp32 emulation against float64 on this case
from tests.test_demix_host import _expand64
from tests.test_export_host import _random_tiled_u
from tests.test_traces_host import _disc, _forms

pytestmark = pytest.mark.gpu
DX = importlib.import_module("localmd_amd.demix")     # the module: localmd_amd.demix is the function it exports
U24 = 2.0 ** -24
ERR_ARG = -2


def _dev(ctx, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- pmd_hals_sweep -------------------------------------------------------------------------------------------------
def _sweep_case(K, seed):
    """CSR rows of a G-like matrix (diagonal stored, not symmetric: the kernel does not care), invd and lo.  Row 0 has no
    off-diagonal entry and is unbounded below (lo = -inf), the last row is coupled to all others; for K >= 3 row 1 has
    invd = 0."""
    rng = np.random.default_rng(seed)
    M = (rng.random((K, K)) < 0.3) * rng.uniform(-0.4, 0.4, (K, K))
    M[0] = 0
    M[-1] = rng.uniform(-0.4, 0.4, K)
    M[np.arange(K), np.arange(K)] = rng.uniform(1, 3, K)
    S = scipy.sparse.csr_matrix(M.astype(np.float32))
    S.sort_indices()
    invd = (1.0 / S.diagonal()).astype(np.float32)
    lo = np.zeros(K, np.float32)
    lo[0] = -np.inf
    if K >= 3:
        invd[1] = 0
    return S, invd, lo


class _Sweep:
    def __init__(self, ctx, S, invd, lo):
        self.ctx, self.K = ctx, S.shape[0]
        self.t = [_dev(ctx, S.indptr.astype(np.int64)), _dev(ctx, S.indices.astype(np.int32)),
                  _dev(ctx, S.data.astype(np.float32)), _dev(ctx, invd), _dev(ctx, lo)]

    def __call__(self, Cd, ldc, Pd, ldp, n, c0=0):
        at = lambda t: C.c_void_p(t.data_ptr() + 4 * c0)   # noqa: E731
        self.ctx.call("pmd_hals_sweep", at(Cd), ldc, at(Pd), ldp, self.K, n, *(ptr(x) for x in self.t))


@pytest.mark.parametrize("K", [1, 3, 70])
def test_sweep_bit_for_bit(gpu_ctx, K):
    S, invd, lo = _sweep_case(K, seed=K)
    run = _Sweep(gpu_ctx, S, invd, lo)
    rng = np.random.default_rng(100 + K)
    for n in (1, 63, 64, 65, 300):
        ldc, ldp = n + 3, n + 7
        C0 = rng.standard_normal((K, ldc)).astype(np.float32)
        P0 = (2 * rng.standard_normal((K, ldp))).astype(np.float32)
        want = C0.copy()
        HR.hals_sweep(want[:, :n], P0[:, :n], S.indptr, S.indices, S.data, invd, lo)   # a view: the padding stays
        Cd, Pd = _dev(gpu_ctx, C0), _dev(gpu_ctx, P0)
        run(Cd, ldc, Pd, ldp, n)
        gpu_ctx.sync()
        got = Cd.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (K, n)
        assert np.array_equal(_bits(got[:, n:]), _bits(C0[:, n:]))                     # the padding beyond n
        if n >= 63:
            assert got[0, :n].min() < 0                                                # lo = -inf lets values go negative
        if K >= 3:
            assert np.array_equal(_bits(got[1]), _bits(C0[1]))                         # invd == 0: untouched
            assert got[2:, :n].min() >= 0
        # a second sweep on the result equals two emulated sweeps
        HR.hals_sweep(want[:, :n], P0[:, :n], S.indptr, S.indices, S.data, invd, lo)
        run(Cd, ldc, Pd, ldp, n)
        gpu_ctx.sync()
        assert np.array_equal(_bits(Cd.cpu().numpy()), _bits(want)), (K, n, "second sweep")
        # the columns in two calls
        if n > 1:
            Cs = _dev(gpu_ctx, C0)
            h = n // 3 + 1
            run(Cs, ldc, Pd, ldp, h)
            run(Cs, ldc, Pd, ldp, n - h, c0=h)
            gpu_ctx.sync()
            assert np.array_equal(_bits(Cs.cpu().numpy()), _bits(got)), (K, n, "split")


def test_sweep_bad_arguments_return_an_error_code(gpu_ctx):
    S, invd, lo = _sweep_case(3, seed=0)
    run = _Sweep(gpu_ctx, S, invd, lo)
    C0 = np.ones((3, 8), np.float32)
    Cd, Pd = _dev(gpu_ctx, C0), _dev(gpu_ctx, C0)
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    tabs = [ptr(x) for x in run.t]
    assert lib.pmd_hals_sweep(h, ptr(Cd), 8, ptr(Pd), 8, 0, 8, *tabs) == ERR_ARG          # K < 1
    assert lib.pmd_hals_sweep(h, ptr(Cd), 8, ptr(Pd), 8, 3, -1, *tabs) == ERR_ARG         # n < 0
    assert lib.pmd_hals_sweep(h, ptr(Cd), 7, ptr(Pd), 8, 3, 8, *tabs) == ERR_ARG          # ldc < n
    assert lib.pmd_hals_sweep(h, ptr(Cd), 8, ptr(Pd), 7, 3, 8, *tabs) == ERR_ARG          # ldp < n
    assert lib.pmd_hals_sweep(h, None, 8, ptr(Pd), 8, 3, 8, *tabs) == ERR_ARG
    assert lib.pmd_hals_sweep(h, ptr(Cd), 8, None, 8, 3, 8, *tabs) == ERR_ARG
    for i in range(5):
        one_null = [None if j == i else t for j, t in enumerate(tabs)]
        assert lib.pmd_hals_sweep(h, ptr(Cd), 8, ptr(Pd), 8, 3, 8, *one_null) == ERR_ARG
    with pytest.raises(PMDLibraryError, match="pmd_hals_sweep"):
        run(Cd, 7, Pd, 8, 8)
    run(Cd, 8, Pd, 8, 0)                                                                   # n == 0: nothing happens
    gpu_ctx.sync()
    assert np.array_equal(Cd.cpu().numpy(), C0)
    z = [ptr(Cd)] * 10
    assert lib.pmd_hals_pixels(h, -1, *z[:9], 4, z[0], 4, z[0]) == ERR_ARG
    assert lib.pmd_hals_pixels(h, 1, None, *z[:8], 4, z[0], 4, z[0]) == ERR_ARG


# ---- pmd_hals_pixels ------------------------------------------------------------------------------------------------
def test_pixels_against_float64(gpu_ctx):
    """Every covering count in {1, 2, 64} on U rows of 0, 1, 63, 64, 65 and 200 nonzeros, a pixel with scale 0, a frozen
    ROI and one with H_kk = 0, and values clamped to exactly 0.

    The bound, derived here: the new value is a_j + (scale sum_i u_i Mt_i - sum_j' a_j' H_j'j) / H_jj.  A term of the
    first sum passes through its product, at most nnz - 1 additions (a lane's chain of ceil(nnz / 64) that starts from an
    exact 0, and the six steps of the butterfly, where adding the exact zero of an idle lane rounds nothing) and the
    scaling; a term of the second
    through its product and fewer than `cover` additions; a_j through none of these.  All of them then share the
    subtraction, the division and the final addition.  No term sees more than nnz + cover + 3 roundings (u = 2^-24), so
    the error of a value is at most (nnz + cover + 3) u sum|terms| with
    sum|terms| = |a_j| + (|scale| sum|u Mt| + sum|a_j' H_j'j|) / H_jj, taken from the float64 run with the values it
    really read (the newest ones).  max(0, .) does not enlarge an error.  The errors of the newer a_j' re-enter through
    H_j'j / H_jj, which the weakly coupled H built here (sum_{j' != j} |H_j'j| <= H_jj / 2) keeps below the room the
    worst-case count leaves."""
    ctx = gpu_ctx
    rng = np.random.default_rng(7)
    K, n_cols = 70, 256
    nnzs, covers = (0, 1, 63, 64, 65, 200), (1, 2, 64)
    rows = []
    for z in nnzs:
        idx = np.sort(rng.choice(n_cols, z, replace=False))
        rows.append((idx, rng.standard_normal(z)))
    U = scipy.sparse.csr_matrix((np.concatenate([r[1] for r in rows]).astype(np.float32),
                                 np.concatenate([r[0] for r in rows]).astype(np.int32),
                                 np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int64)),
                                shape=(len(nnzs), n_cols))
    FROZEN, DEAD = 5, 9
    px_row, cov, scale = [], [], []
    for r in range(len(nnzs)):
        for c in covers:
            ks = np.sort(rng.choice(K, c, replace=False))
            if c == 64:
                ks = np.union1d(np.setdiff1d(ks, [FROZEN, DEAD])[:62], [FROZEN, DEAD])
            px_row.append(r), cov.append(ks), scale.append(rng.uniform(0.5, 2))
    px_row.append(5), cov.append(np.array([1, 2, 3])), scale.append(0.0)        # scale == 0
    n_px = len(px_row)
    cov_ptr = np.concatenate([[0], np.cumsum([len(k) for k in cov])]).astype(np.int64)
    cov_k = np.concatenate(cov).astype(np.int32)
    a0 = rng.uniform(0, 1, len(cov_k)).astype(np.float32)
    ldm, ldh = n_cols + 5, K + 3
    Mt = np.zeros((K, ldm), np.float32)
    Mt[:, :n_cols] = rng.standard_normal((K, n_cols)) * 0.2 - 0.05             # a negative drift: some values clamp at 0
    off = rng.uniform(-1, 1, (K, K)) / (2 * K)
    Hm = (off + off.T) / 2 + np.diag(rng.uniform(1, 2, K))
    Hm[DEAD, :] = Hm[:, DEAD] = 0
    H = np.zeros((K, ldh), np.float32)
    H[:, :K] = Hm
    frozen = np.zeros(K, np.int32)
    frozen[FROZEN] = 1
    scale = np.asarray(scale, np.float32)
    px_row = np.asarray(px_row, np.int32)

    a_dev = _dev(ctx, a0)
    args = [_dev(ctx, x) for x in (px_row, cov_ptr, cov_k)] + [a_dev] + [_dev(ctx, x) for x in (
        U.indptr.astype(np.int64), U.indices.astype(np.int32), U.data.astype(np.float32), scale, Mt)]
    Hd, fd = _dev(ctx, H), _dev(ctx, frozen)
    ctx.call("pmd_hals_pixels", n_px, *(ptr(x) for x in args), ldm, ptr(Hd), ldh, ptr(fd))
    ctx.sync()
    got = a_dev.cpu().numpy()

    H64, Mt64 = H[:, :K].astype(np.float64), Mt[:, :n_cols].astype(np.float64)
    want = HR.hals_pixels(a0.astype(np.float64), px_row, cov_ptr, cov_k, U.astype(np.float64), scale.astype(np.float64),
                          Mt64, H64, frozen)
    skipped = np.isin(cov_k, [FROZEN, DEAD])
    assert np.array_equal(_bits(got[skipped]), _bits(a0[skipped]))             # frozen / H_kk == 0: bitwise unchanged
    assert np.any(got[~skipped] != a0[~skipped])
    clamped = 0
    ref = a0.astype(np.float64)               # replayed pair by pair to collect sum|terms| of every update
    for q in range(n_px):
        j0, j1 = int(cov_ptr[q]), int(cov_ptr[q + 1])
        ks = cov_k[j0:j1]
        s, e = U.indptr[px_row[q]], U.indptr[px_row[q] + 1]
        nnz, cover = e - s, j1 - j0
        Hs = H64[np.ix_(ks, ks)]
        sy_abs = abs(float(scale[q])) * (np.abs(Mt64[ks][:, U.indices[s:e]]) @ np.abs(U.data[s:e].astype(np.float64)))
        for j in range(cover):
            if ks[j] in (FROZEN, DEAD):
                continue
            terms = abs(ref[j0 + j]) + (sy_abs[j] + np.abs(ref[j0:j1]) @ np.abs(Hs[:, j])) / Hs[j, j]
            ref[j0 + j] = want[j0 + j]        # the value the pairs after j read
            err = abs(float(got[j0 + j]) - want[j0 + j])
            assert err <= (nnz + cover + 3) * U24 * terms, (q, nnz, cover, j, err, terms)
            clamped += int(got[j0 + j] == 0 and want[j0 + j] == 0)
    assert clamped >= 3
    assert np.all(got >= 0)
    # a second call goes on from the result
    ctx.call("pmd_hals_pixels", n_px, *(ptr(x) for x in args), ldm, ptr(Hd), ldh, ptr(fd))
    ctx.sync()
    want2 = HR.hals_pixels(want.copy(), px_row, cov_ptr, cov_k, U.astype(np.float64), scale.astype(np.float64), Mt64, H64,
                           frozen)
    got2 = a_dev.cpu().numpy()
    assert np.array_equal(_bits(got2[skipped]), _bits(a0[skipped])) and np.all(got2 >= 0)
    assert np.abs(got2 - want2).max() <= 2 * (200 + 64 + 3) * U24 * max(1.0, np.abs(want2).max())


# ---- demix end to end ----------------------------------------------------------------------------------------------
T, D1, D2, RANK = 300, 24, 20, 12


def _pmd(order, T=T, seed=4):
    """A decomposition-shaped PMDArray; the C-order one holds the same movie as the F-order one (U's rows permuted)."""
    u = _random_tiled_u(D1, D2, 12, 10, "F", 1, seed=seed)
    if order == "C":
        u = u[np.arange(D1 * D2).reshape((D1, D2), order="F").reshape(-1)]        # row of C-order pixel c
    rng = np.random.default_rng(seed + 2)
    k = u.shape[1]
    return PMDArray(scipy.sparse.csr_matrix(u), (rng.standard_normal((k, RANK)) * 0.1).astype(np.float32),
                    np.linspace(20, 2, RANK).astype(np.float32),
                    (rng.standard_normal((RANK, T)) * 0.05 + rng.uniform(-0.02, 0.02, (RANK, 1))).astype(np.float32),
                    (T, D1, D2), order, rng.uniform(500, 1500, (D1, D2)).astype(np.float32),
                    rng.uniform(2, 10, (D1, D2)).astype(np.float32))


def _rois():
    """4 discs, of which the first two overlap, and the whole field."""
    m = np.stack([_disc(D1, D2, 6, 6, 3.6), _disc(D1, D2, 8, 9, 3.6), _disc(D1, D2, 17, 5, 3.1), _disc(D1, D2, 16, 14, 2.4),
                  np.ones((D1, D2), bool)])
    assert (m[0] & m[1]).sum() >= 5 and not (m[2] & m[3]).any() and not (m[0] & m[2]).any()
    return m


def _same(a, b):
    """True when every output of the two results has the same bits; else the assertion names the first that differs."""
    assert np.array_equal(a.empty, b.empty), "empty"
    assert np.array_equal(_bits(a.traces), _bits(b.traces)), ("traces", np.abs(a.traces - b.traces).max())
    assert np.array_equal(_bits(a.footprints.toarray()), _bits(b.footprints.toarray())), "footprints"
    assert np.array_equal(_bits(a.background), _bits(b.background)), "background"
    assert np.array_equal(a.objective, b.objective), ("objective", a.objective - b.objective)
    return True


@pytest.fixture(scope="module")
def e2e(gpu_ctx):
    """The F-order case, its device result and the float64 reference, computed once."""
    pmd = _pmd("F")
    rois = _rois()
    X = _expand64(pmd)
    S = rois.reshape(len(rois), -1).T
    ref = HR.demix_ref(X, S.astype(np.float64), S)
    return pmd, rois, X, ref, localmd_amd.demix(pmd, rois, ctx=gpu_ctx)


# the same measurement for the two traces-only calls of test_traces_only (allowed: 4 x)
REF32_FIXED = {"traces": 4.56e-7, "objective": 5.15e-7}      # outer_iters=3, sweeps=2, update_footprints=False
REF32_UNBOUNDED = {"traces": 6.13e-7}                        # outer_iters=1, sweeps=2, fixed footprints, nonneg_traces=False


def test_demix_against_the_float64_reference(e2e):
    pmd, rois, X, ref, dm = e2e
    assert dm.traces.shape == (5, T) and dm.traces.dtype == np.float32
    assert scipy.sparse.issparse(dm.footprints) and dm.footprints.shape == (5, D1 * D2) and dm.footprints.dtype == np.float32
    assert dm.background.shape == (D1, D2) and dm.background.dtype == np.float32
    assert dm.objective.shape == (3,) and dm.objective.dtype == np.float64 and dm.empty.dtype == bool
    assert np.array_equal(dm.labels, np.arange(5))
    got = {"traces": dm.traces, "footprints": dm.footprints.toarray().T, "background": dm.background.reshape(-1),
           "objective": dm.objective}
    for key, fp32 in REF32.items():
        rel = _rel(got[key], ref[key])
        print(key, "device vs float64:", rel, "allowed:", 4 * fp32)
    for key, fp32 in REF32.items():
        assert _rel(got[key], ref[key]) <= 4 * fp32, key
    assert np.all(np.diff(dm.objective) <= 0)
    assert np.array_equal(dm.empty, ref["empty"])
    assert np.all(dm.footprints.data >= 0) and np.array_equal(dm.traces.min(axis=1), np.zeros(5, np.float32))
    assert np.array_equal(dm.footprints.toarray() != 0, rois.reshape(5, -1) & (dm.footprints.toarray() != 0))


def test_traces_only(gpu_ctx, e2e):
    pmd, rois, X, ref, _ = e2e
    a = localmd_amd.demix(pmd, rois, outer_iters=3, sweeps=2, update_footprints=False, ctx=gpu_ctx)
    b = pmd.demix(rois, outer_iters=1, sweeps=4, update_footprints=False, ctx=gpu_ctx)
    # the footprints stay at their normalised input ...
    W, _ = roi_weights(rois, (D1, D2), "F")
    assert np.array_equal(_bits(a.footprints.data), _bits(DX.unit_columns(W).astype(np.float32)))
    assert np.array_equal(a.footprints.indices, W.indices) and not a.empty.any()
    # ... and the traces are one temporal solve: 8 sweeps in a row, however they are spread over outer iterations
    assert np.array_equal(_bits(a.traces), _bits(b.traces)) and np.array_equal(_bits(a.background), _bits(b.background))
    assert a.objective[-1] == b.objective[-1] and np.all(np.diff(a.objective) <= 0)
    S = rois.reshape(5, -1).T
    r = HR.demix_ref(X, S.astype(np.float64), S, outer_iters=3, sweeps=2, update_footprints=False)
    assert _rel(a.traces, r["traces"]) <= 4 * REF32_FIXED["traces"]
    assert _rel(a.objective, r["objective"]) <= 4 * REF32_FIXED["objective"]
    # unbounded traces: not shifted, some negative
    c = localmd_amd.demix(pmd, rois, outer_iters=1, sweeps=2, update_footprints=False, nonneg_traces=False, ctx=gpu_ctx)
    r = HR.demix_ref(X, S.astype(np.float64), S, outer_iters=1, sweeps=2, update_footprints=False, nonneg_traces=False)
    assert c.traces.min() < 0 and _rel(c.traces, r["traces"]) <= 4 * REF32_UNBOUNDED["traces"]


def test_same_bits_for_residency_order_and_roi_form(gpu_ctx, e2e):
    pmd, rois, _, _, dm = e2e
    pmd.to_device(ctx=gpu_ctx)
    try:
        assert _same(localmd_amd.demix(pmd, rois), dm)
    finally:
        pmd.to_host()
    pc = _pmd("C")
    assert np.array_equal(pc[:5], pmd[:5])
    assert _same(localmd_amd.demix(pc, rois, ctx=gpu_ctx), dm)
    for order, p in (("F", pmd), ("C", pc)):
        for name, form in _forms(rois.astype(np.float64), order).items():
            assert _same(localmd_amd.demix(p, form, ctx=gpu_ctx), dm), (order, name)


def test_label_image_ties_demix_to_extract_traces(gpu_ctx, e2e):
    """ROIs that do not overlap, one sweep per step and fixed footprints: G is diagonal, so the two sweeps of the call
    (the start and the one outer iteration) have the closed form C_k = max(0, (tr_k - A_k mean + o_k) / G_kk) with tr the
    extract_traces(..., reduce="sum") rows of the normalised footprints and o = -Wk vbar + G cbar, cbar = 0 in the first
    sweep and the first sweep's row means in the second; then the shift.  Each value is a few fp32 operations on tr: the
    allowance is 8 u of the largest term."""
    pmd, rois, X, _, _ = e2e
    lab = np.zeros((D1, D2), np.int64)
    for k in (0, 2, 3):
        lab[rois[k]] = 10 * (k + 1)
    dm = localmd_amd.demix(pmd, lab, outer_iters=1, sweeps=1, update_footprints=False, ctx=gpu_ctx)
    assert np.array_equal(dm.labels, [10, 30, 40])
    masks = rois[[0, 2, 3]]
    assert _same(dm, localmd_amd.demix(pmd, masks, outer_iters=1, sweeps=1, update_footprints=False, ctx=gpu_ctx)) is True
    W, _ = roi_weights(masks, (D1, D2), "F")
    A = scipy.sparse.csr_matrix((DX.unit_columns(W).astype(np.float32).astype(np.float64), W.indices, W.indptr),
                                shape=W.shape).toarray()              # the footprints demix holds, exactly
    tr = localmd_amd.extract_traces(pmd, A.reshape(3, D1, D2), reduce="sum", ctx=gpu_ctx).denoised.astype(np.float64)
    gkk = (A * A).sum(axis=1)
    mean = np.asarray(pmd.mean_img, np.float64).reshape(-1)
    qv, mbar = DX.time_mean_factors(pmd)
    wkv = tr - (A @ mean)[:, None]                       # Wk V
    wkvbar = A @ (mbar - mean)                           # Wk vbar
    c1 = np.maximum(0, (wkv - wkvbar[:, None]) / gkk[:, None])
    c2 = np.maximum(0, (wkv + (-wkvbar + gkk * c1.mean(axis=1))[:, None]) / gkk[:, None])
    want = c2 - c2.min(axis=1, keepdims=True)
    big = np.abs(tr).max() / gkk.min()
    assert np.abs(dm.traces - want).max() <= 8 * U24 * big
    assert np.abs(dm.background.reshape(-1) - (mbar - A.T @ want.mean(axis=1))).max() <= 8 * U24 * max(big, np.abs(mbar).max())


def _planted_pmd(seed=3, T=300, d1=16, d2=16):
    """A noiseless rank-2 movie of two overlapping cells with distinct traces on a static background, as a PMDArray."""
    rng = np.random.default_rng(seed)
    masks = np.stack([_disc(d1, d2, 6, 6, 3.6), _disc(d1, d2, 8, 9, 3.6)])
    ii, jj = np.mgrid[0:d1, 0:d2]
    foot = np.stack([masks[0] * np.exp(-((ii - 6) ** 2 + (jj - 6) ** 2) / 12.0),
                     masks[1] * np.exp(-((ii - 8) ** 2 + (jj - 9) ** 2) / 12.0)])
    traces = np.zeros((2, T))
    for k in range(2):
        for t0 in rng.choice(T - 30, 8, replace=False):
            traces[k, t0:t0 + 30] += rng.uniform(0.5, 2) * np.exp(-np.arange(30) / 6.0)
    std = rng.uniform(1, 2, (d1, d2))
    u = scipy.sparse.csr_matrix((foot.reshape(2, -1) / std.reshape(1, -1)).T)        # D x 2, rows in C order
    pmd = PMDArray(u, np.eye(2, dtype=np.float32), np.ones(2, np.float32), traces.astype(np.float32), (T, d1, d2), "C",
                   rng.uniform(5, 10, (d1, d2)).astype(np.float32), std.astype(np.float32))
    return pmd, masks, traces


def _corr(a, b):
    return np.array([np.corrcoef(a[k], b[k])[0, 1] for k in range(len(a))])


def test_planted_overlapping_cells_are_demixed(gpu_ctx):
    """Checked on the CPU with demix_ref on this seed: the reference's traces correlate with the planted ones at
    0.99999996 and 0.99999997, the mask averages at 0.936 and 0.931."""
    pmd, masks, traces = _planted_pmd()
    dm = localmd_amd.demix(pmd, masks, ctx=gpu_ctx)
    mix = localmd_amd.extract_traces(pmd, masks, ctx=gpu_ctx).denoised
    c_dm, c_mix = _corr(dm.traces, traces), _corr(mix, traces)
    print("demix", c_dm, "extract_traces", c_mix)
    assert np.all(c_dm > c_mix) and np.all(c_dm >= 0.99)
    assert np.all(c_mix < 0.99)


def test_device_memory_grows_as_8_k_t(gpu_ctx):
    import torch

    rois = _rois()
    K = len(rois)
    peak = {}
    for n in (300, 1200):
        pmd = _pmd("F", T=n)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(gpu_ctx.device)
        torch.cuda.reset_peak_memory_stats(gpu_ctx.device)
        localmd_amd.demix(pmd, rois, outer_iters=1, sweeps=1, ctx=gpu_ctx)
        peak[n] = torch.cuda.max_memory_allocated(gpu_ctx.device) - base
    slack = 1 << 20                        # the plan's allowance for the allocator's rounding of the small arrays
    assert peak[1200] - peak[300] <= 8 * K * 900 + slack, peak
    W, _ = roi_weights(rois, (D1, D2), "F")
    pmd = _pmd("F", T=1200)
    plan = DX.demix_device_bytes(K=K, T=1200, n_pairs=W.nnz, n_px=D1 * D2, nnz_g=K * K, nnz_b=K * pmd.u.shape[1],
                                 nnz_u=pmd.u.nnz, n_rows=D1 * D2, n_cols=pmd.u.shape[1], rank=RANK, factors_on_device=False)
    assert peak[1200] <= plan, (peak, plan)
