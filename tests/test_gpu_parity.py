"""
Stage-level and end-to-end parity tests (GPU): the HIP path, called through the C ABI and the
Python host mirror, against the CPU oracle on identical seeded inputs (the oracle consumes the
Gaussian matrices the device generated).  Tolerances are stated per quantity; integer outputs
(tile ranks, CSR structure) must be bit-exact unless a decision statistic sits within
KNIFE_EDGE of its threshold, in which case the tile is reported and excused.
"""
import numpy as np
import pytest

from oracle import pmd_oracle as O, philox
from tests.util import DeviceSource, sign_align, rel_err
from tests import parity_metrics as PM

pytestmark = pytest.mark.gpu
KNIFE_EDGE = 2e-3


def _t():
    import torch

    return torch


def P(t):
    from localmd_amd._lib import ptr

    return ptr(t)


def dev(ctx, a):
    torch = _t()
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _movie(T, d1, d2, seed=1):
    from localmd_amd.synthetic import make_movie

    return make_movie(T, d1, d2, seed=seed)


@pytest.mark.parametrize("T,compute_normalizer", [(2100, True), (1300, True), (200, True), (700, False)])
def test_stats_mean_and_welch_noise(gpu_ctx, T, compute_normalizer):
    torch = _t()
    ctx = gpu_ctx
    d1, d2 = 23, 31
    mov = _movie(T, d1, d2, seed=3)
    D = d1 * d2
    md = dev(ctx, mov.reshape(T, D))
    mean = torch.empty(D, dtype=torch.float32, device=ctx.device)
    std = torch.empty(D, dtype=torch.float32, device=ctx.device)
    ws = ctx.workspace(ctx.lib.pmd_stats_workspace_bytes(T, D, 1024))
    ctx.call("pmd_stats", P(md), T, D, 1024, 1 if compute_normalizer else 0, P(mean), P(std), P(ws), ws.numel())
    ctx.sync()
    np.random.seed(0)
    loader = O.PMDLoader(mov, philox.PhiloxSource(0), background_rank=0, compute_normalizer=compute_normalizer)
    np.testing.assert_allclose(mean.cpu().numpy().reshape(d1, d2), loader.mean_img, rtol=1e-5)
    np.testing.assert_allclose(std.cpu().numpy().reshape(d1, d2), loader.std_img, rtol=2e-4)


def test_standardize_filter_project(gpu_ctx):
    torch = _t()
    ctx = gpu_ctx
    T, d1, d2, K = 300, 20, 18, 3
    rng = np.random.default_rng(0)
    mov = _movie(T, d1, d2, seed=4)
    D = d1 * d2
    mean = mov.mean(axis=0).astype(np.float32)
    std = (mov.std(axis=0) + 0.5).astype(np.float32)
    basis_f, _ = np.linalg.qr(rng.standard_normal((D, K)))
    basis_f = basis_f.astype(np.float32)             # rows in F order
    fov = np.arange(D).reshape((d1, d2), order="F")
    basis_c = basis_f[fov.reshape(-1)]                # rows in C order
    frames = sorted(rng.choice(T, size=120, replace=False).tolist())
    rows = 1024
    ld = ctx.lib.pmd_time_ld(len(frames))
    xs = torch.zeros((rows, ld), dtype=torch.float32, device=ctx.device)
    md, fr = dev(ctx, mov.reshape(T, D)), dev(ctx, np.asarray(frames, dtype=np.int32))
    mu, sg, bd = dev(ctx, mean.reshape(-1)), dev(ctx, std.reshape(-1)), dev(ctx, basis_c)
    ctx.call("pmd_standardize_transpose", P(md), D, P(fr), len(frames), P(mu), P(sg), P(xs), ld)
    pj = torch.zeros((K, ld), dtype=torch.float32, device=ctx.device)
    ws = ctx.workspace(ctx.lib.pmd_bg_project_workspace_bytes(D, len(frames)))
    ctx.call("pmd_bg_project", P(xs), D, len(frames), ld, P(bd), K, P(pj), ld, P(ws), ws.numel())
    xf = torch.zeros_like(xs)
    ctx.call("pmd_bg_filter", P(xs), P(xf), D, len(frames), ld, P(bd), K, P(pj), ld)
    ctx.sync()
    crop = mov[frames].transpose(1, 2, 0)
    ref, tp = O.standardize_and_filter(crop, mean, std, basis_f.reshape((d1, d2, K), order="F"))
    got = xf.cpu().numpy()[:D, : len(frames)].reshape(d1, d2, -1)
    np.testing.assert_allclose(pj.cpu().numpy()[:, : len(frames)], tp, rtol=0, atol=2e-4 * np.abs(tp).max())
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-5 * np.abs(ref).max())
    assert np.all(xs.cpu().numpy()[:D, len(frames):] == 0)


def test_background_rsvd(gpu_ctx):
    torch = _t()
    ctx = gpu_ctx
    T, d1, d2, K = 400, 24, 30, 4
    mov = _movie(T, d1, d2, seed=5)
    D = d1 * d2
    rng = np.random.default_rng(1)
    xs_np = rng.standard_normal((D, 6)) @ (np.linspace(30, 5, 6)[:, None] * rng.standard_normal((6, T)))
    xs_np = (xs_np + 0.5 * rng.standard_normal((D, T))).astype(np.float32)
    ld = ctx.lib.pmd_time_ld(T)
    xs = torch.zeros((1024, ld), dtype=torch.float32, device=ctx.device)
    xs[:D, :T] = dev(ctx, xs_np)
    seed = 77
    basis = torch.empty((D, K), dtype=torch.float32, device=ctx.device)
    ws = ctx.workspace(ctx.lib.pmd_background_rsvd_workspace_bytes(D, T, K))
    ctx.call("pmd_background_rsvd", P(xs), D, T, ld, K, seed, P(basis), P(ws), ws.numel())
    ctx.sync()
    src = DeviceSource(ctx, seed)
    omega = src.omega(philox.STREAM_BG_OMEGA, 0, T, K + 10)
    ref, _ = O.loader_truncated_random_svd(xs_np, omega, K)
    got = basis.cpu().numpy()
    assert np.abs(got.T @ got - np.eye(K)).max() < 1e-5
    got = sign_align(got, ref)
    assert rel_err(got, ref) < 2e-4


def test_threshold_simulation(gpu_ctx):
    torch = _t()
    ctx = gpu_ctx
    b1, b2, t, iters, seed = 20, 20, 500, 12, 5
    ws = ctx.workspace(ctx.lib.pmd_threshold_sim_workspace_bytes(b1, b2, t, iters))
    out = torch.empty((iters, 2), dtype=torch.float32, device=ctx.device)
    ctx.call("pmd_threshold_sim", b1, b2, t, iters, seed, P(out), P(ws), ws.numel())
    ctx.sync()
    got = out.cpu().numpy()
    src = DeviceSource(ctx, seed)
    _, _, sp, tp = O.threshold_heuristic([b1, b2, t], src, num_comps=1, iters=iters, percentile_threshold=5)
    np.testing.assert_allclose(got[:, 0], sp, rtol=2e-4)
    np.testing.assert_allclose(got[:, 1], tp, rtol=2e-4)


def _run_tiles(ctx, xf_np, d1, d2, b1, b2, r, a, thr, seed):
    """xf_np: (d1, d2, Tcrop) filtered standardised movie.  Returns device outputs as numpy."""
    torch = _t()
    from localmd_amd import grid

    lib = ctx.lib
    Tc = xf_np.shape[2]
    D = d1 * d2
    ld = lib.pmd_time_ld(Tc)
    xf = torch.zeros((D, ld), dtype=torch.float32, device=ctx.device)
    xf[:, :Tc] = dev(ctx, xf_np.reshape(D, Tc))
    it1, it2 = grid.tile_origins((d1, d2), (b1, b2))
    pix, origins = grid.tile_pixel_lists((d1, d2), (b1, b2), it1, it2)
    pool_q, pool_idx, pool_w, _ = grid.pooling_maps((b1, b2), 2)
    n = pix.shape[0]
    d = b1 * b2
    dpad = lib.pmd_tile_dpad(d)
    Pn = pool_q.shape[0]
    ut = torch.empty((n, 64, dpad), dtype=torch.float32, device=ctx.device)
    v = torch.empty((n, 64, ld), dtype=torch.float32, device=ctx.device)
    stats = torch.zeros((n, 64, 2), dtype=torch.float32, device=ctx.device)
    good = torch.zeros((n, 64), dtype=torch.int32, device=ctx.device)
    keep = torch.zeros((n, 64), dtype=torch.int32, device=ctx.device)
    ranks = torch.zeros((n,), dtype=torch.int32, device=ctx.device)
    lam = torch.zeros((n, 64), dtype=torch.float64, device=ctx.device)
    ws = ctx.workspace(lib.pmd_tiles_workspace_bytes(n, b1, b2, Pn, r, a, Tc, ld, D))
    pix_d, pq_d, pi_d, pw_d = dev(ctx, pix), dev(ctx, pool_q), dev(ctx, pool_idx), dev(ctx, pool_w)
    ctx.call("pmd_tiles_decompose", P(xf), ld, D, Tc, P(pix_d), n, b1, b2, P(pq_d), pool_q.shape[1], Pn,
             P(pi_d), P(pw_d), r, a, float(thr[0]), float(thr[1]), 1, seed, 0, 1, P(ut), P(v), ld,
             P(stats), P(good), P(keep), P(ranks), P(lam), P(ws), ws.numel())
    ctx.sync()
    return dict(ut=ut.cpu().numpy(), v=v.cpu().numpy()[:, :, :Tc], stats=stats.cpu().numpy(), good=good.cpu().numpy(),
                keep=keep.cpu().numpy(), ranks=ranks.cpu().numpy(), lam=lam.cpu().numpy(), origins=origins, n=n)


@pytest.mark.parametrize("b1,b2,r,T", [(20, 20, 8, 600), (16, 24, 6, 400), (32, 32, 10, 300), (20, 20, 10, 100)])
def test_tiles_decompose_vs_oracle(gpu_ctx, b1, b2, r, T):
    ctx = gpu_ctx
    d1, d2, a, seed = b1 + b1 // 2 + 3, b2 + b2 // 2, 10, 11
    mov = _movie(T, d1, d2, seed=9).astype(np.float32)
    x = (mov - mov.mean(axis=0)) / 1.0
    xf = np.ascontiguousarray(x.transpose(1, 2, 0))  # (d1, d2, T)
    thr = (1.3, 2.3)
    out = _run_tiles(ctx, xf, d1, d2, b1, b2, r, a, thr, seed)
    src = DeviceSource(ctx, seed)
    d = b1 * b2
    for t, (k, j) in enumerate(out["origins"]):
        block = xf[k:k + b1, j:j + b2, :]
        omega = src.omega(philox.STREAM_TILE_OMEGA, t, T // a, r + 10)
        u_ref, good_ref, v_ref, st = O.single_block_md(block, omega, r, a, 2, thr[0], thr[1])
        u_ref2 = u_ref.reshape((d, r), order="F")
        # singular values (sigma) and statistics
        sig_ref = np.linalg.norm(v_ref, axis=1)
        sig = np.sqrt(np.maximum(out["lam"][t, :r], 0))
        strong = sig_ref > 1e-3 * sig_ref[0]
        np.testing.assert_allclose(sig[strong], sig_ref[strong], rtol=2e-4)
        # components with well separated singular values agree after sign alignment
        gaps = np.minimum(np.abs(np.diff(sig_ref, prepend=np.inf)), np.abs(np.diff(sig_ref, append=0))) / sig_ref
        sep = (gaps > 2e-2) & strong
        u_got = out["ut"][t, :r, :d].T
        v_got = out["v"][t, :r, :]
        u_al = sign_align(u_got, u_ref2)
        v_al = sign_align(v_got, v_ref, axis=1)
        for c in np.nonzero(sep)[0]:
            tol = 6e-5 * sig_ref[0] / (gaps[c] * sig_ref[c]) + 2e-4  # fp32 perturbation / relative gap
            assert rel_err(u_al[:, c], u_ref2[:, c]) < tol, (t, c, gaps[c])
            assert rel_err(v_al[c], v_ref[c]) < tol, (t, c, gaps[c])
        # the spanned subspace of all strong components agrees
        ns = int(strong.sum())
        proj = u_ref2[:, :ns] @ (u_ref2[:, :ns].T @ u_got[:, :ns])
        assert rel_err(proj, u_got[:, :ns]) < 5e-3
        assert np.abs(u_got[:, :ns].T @ u_got[:, :ns] - np.eye(ns)).max() < 2e-5
        # decisions: bit-exact unless a statistic is within KNIFE_EDGE of its threshold
        sp, tp = st["spatial"], st["temporal"]
        margin = np.minimum(np.abs(sp - thr[0]) / thr[0], np.abs(tp - thr[1]) / thr[1])
        kept_ref = O.filter_by_failures(good_ref.flatten() > 0, 1)
        rank_ref = int(kept_ref.sum())
        evaluated = np.arange(r) < rank_ref
        if np.all(margin[evaluated] > KNIFE_EDGE):
            assert out["ranks"][t] == rank_ref, (t, sp, tp, out["stats"][t, :r])
            np.testing.assert_array_equal(out["keep"][t, :r] > 0, kept_ref)
        np.testing.assert_allclose(out["stats"][t, :rank_ref, 0][sep[:rank_ref]], sp[:rank_ref][sep[:rank_ref]], rtol=5e-3)
        np.testing.assert_allclose(out["stats"][t, :rank_ref, 1][sep[:rank_ref]], tp[:rank_ref][sep[:rank_ref]], rtol=5e-3)


def _compare_full(ctx, mov, block, frame_range, **kw):
    import localmd_amd
    from localmd_amd import decomposition as Dm

    Dm.QUIET = True
    seed = kw.pop("seed", 123)
    np.random.seed(7)
    pmd, diag = localmd_amd.localmd_decomposition(mov, block, frame_range, seed=seed, return_diagnostics=True, ctx=ctx, **kw)
    np.random.seed(7)
    okw = {k: v for k, v in kw.items() if k not in ("sim_iters", "thresholds", "orthogonalizer", "null_directions", "null_cutoff")}
    ref = O.localmd_decomposition(mov, block, frame_range, rng=DeviceSource(ctx, seed),
                                  thresholds=diag["thresholds"], **okw)
    return pmd, diag, ref


def _check_full(pmd, diag, ref, mov, vt_tol=1e-3, orth_tol=2e-3, s_tol=5e-4, vt_tol_signal=1e-4, u_tol=5e-4, r_tol=None,
                probe_tol=2e-3):
    """Tolerances: s_tol relative on the resolvable singular values (with the (s_1/s_c)^2 eps growth of a Gram-matrix
    SVD); vt_tol_signal = Frobenius error of the Vt rows of the signal components (the north-star figure, 1e-4 where
    R <= frames); u_tol = |U_data diff| on the stable tile columns relative to max |U_data|; r_tol (default 20 x
    vt_tol_signal) = |R diff| on stable rows x signal columns relative to max |R|; orth_tol on the resolvable
    strong components (s > 5 % of s_1), plus a bound of 1e-5 on the deviation weighted by s_c s_c' / s_1^2 over all resolvable
    ones (the residual of an fp32 Gram eigendecomposition is ~eps lambda_1 ~ 1e-7; tests/parity_metrics.py defines the classes)."""
    T, d1, d2 = mov.shape
    assert diag["frames"] == ref.diag["frames"]
    np.testing.assert_allclose(pmd.mean_img, ref.mean_img, rtol=1e-5)
    np.testing.assert_allclose(pmd.var_img, ref.std_img, rtol=2e-4)
    # tile ranks / CSR structure: bit exact outside knife-edge tiles
    ranks_ref = ref.diag["tile_ranks"]
    thr = diag["thresholds"]
    knife = []
    for t, dl in enumerate(ref.diag["tile_diag"]):
        d0 = dl[0]
        n_eval = int(ranks_ref[t])
        m = np.minimum(np.abs(d0["spatial"][:n_eval] - thr[0]) / thr[0], np.abs(d0["temporal"][:n_eval] - thr[1]) / thr[1])
        if np.any(m < KNIFE_EDGE):
            knife.append(t)
    mism = np.nonzero(diag["tile_ranks"] != ranks_ref)[0].tolist()
    assert set(mism) <= set(knife), (mism, knife)
    exact = len(mism) == 0
    if exact:
        # same shapes as the reference on every route (decomposition.py:984-988 keeps every non-zero direction)
        assert pmd.u.shape == ref.u.shape
        assert pmd.r.shape == ref.r.shape and pmd.s.shape == ref.s.shape and pmd.v.shape == ref.v.shape, \
            (pmd.r.shape, ref.r.shape, pmd.s.shape, ref.s.shape)
        np.testing.assert_array_equal(pmd.u.indptr, ref.u.indptr)
        np.testing.assert_array_equal(pmd.u.indices, ref.u.indices)
        m = PM.measure(pmd, ref, PM.hip_cols(diag), PM.oracle_cols(ref), diag["n_tile_cols"])
    else:
        m = PM.measure(pmd, ref)
    # orthonormality of [UR] and Vt over the resolvable components
    assert m["orth_ur"][0] < orth_tol, m["orth_ur"]
    assert m["orth_vt"][0] < orth_tol, m["orth_vt"]
    assert m["orth_ur_weighted"][0] < 1e-5 and m["orth_vt_weighted"][0] < 1e-5, (m["orth_ur_weighted"], m["orth_vt_weighted"])
    # reconstruction on random probes (independent of sign / rotation ambiguities)
    assert PM.probes(pmd, ref, mov.shape, n=400) < probe_tol
    if exact:
        # U_data on the stable tile columns, R on stable rows x signal columns (element-wise, after sign alignment)
        assert m["u_data_err_stable"] < u_tol * m["u_data_max_abs"], (m["u_data_err_stable"], m["u_data_max_abs"])
        rt = 20 * vt_tol_signal if r_tol is None else r_tol
        assert m["r_err_stable_signal"] < rt * m["r_max_abs"], (m["r_err_stable_signal"], m["r_max_abs"])
        n = len(m["s_rel"])
        valid, sep, sig = m["valid"], m["sep"], m["signal"]
        # sigma comes from an fp32 Gram eigendecomposition on both sides: lambda_c carries an absolute error of
        # ~eps lambda_1, i.e. sigma_c a relative error of ~eps (sigma_1 / sigma_c)^2
        s_rtol = np.maximum(s_tol, 1e-6 * (ref.s[0] / ref.s[:n]) ** 2)
        assert np.all(m["s_rel"][valid] <= s_rtol[valid]), np.max(m["s_rel"][valid])
        # (a) north-star criterion: Vt Frobenius error on the signal components (sigma > 5% of sigma_1, separated
        #     from their neighbours) that are well conditioned for an fp32 Gram-based SVD (which both sides are): a
        #     right vector carries an error of ~eps (sigma_1/sigma_c)^2 / gap_c in either implementation; components
        #     where that alone exceeds 2e-5 cannot be expected to agree to 1e-4 and are covered by (b)
        cond = 6e-8 * (ref.s[0] / ref.s[:n]) ** 2 / np.maximum(m["gaps"], 1e-12)
        wc = sig & (cond < 2e-5)
        va = sign_align(pmd.v[:n], ref.v[:n], axis=1)
        if wc.any():
            err_sig = np.linalg.norm(va[wc] - ref.v[:n][wc]) / np.linalg.norm(ref.v[:n][wc])
            assert err_sig < vt_tol_signal, err_sig
        # (b) every separated component within the first-order perturbation bound eps * sigma_1 / (sigma_c * gap_c)
        for c in np.nonzero(sep)[0]:
            assert m["vt_row_err"][c] < vt_tol * 2e-2 * ref.s[0] / (ref.s[c] * m["gaps"][c]) + 2e-4, (c, m["vt_row_err"][c], m["gaps"][c], ref.s[c])
    return exact, knife


def test_full_pipeline_small(gpu_ctx):
    mov = _movie(600, 40, 50, seed=1)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (20, 20), 600, max_components=6, background_rank=2, sim_iters=20)
    _check_full(pmd, diag, ref, mov)
    # thresholds: device simulation vs oracle simulation on the same noise
    _, _, sp, tp = O.threshold_heuristic([20, 20, 600], DeviceSource(gpu_ctx, 123), iters=20)
    np.testing.assert_allclose(diag["sim_stats"][:, 0], sp, rtol=2e-4)
    np.testing.assert_allclose(diag["sim_stats"][:, 1], tp, rtol=2e-4)


def test_full_pipeline_max_components_80(gpu_ctx):
    """max_components is unbounded in the reference (decomposition.py:643-665; the rSVD at :59-67 takes any rank): beyond
    54 the sketch (max_components + 10 columns) no longer fits the 64 component rows of the MFMA-tiled kernels and the tile
    stage runs the generic-width kernels (csrc/wide.hip) on 128-row arrays.  Same checks as every other configuration."""
    mov = _movie(1200, 40, 50, seed=21)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (20, 20), 1200, max_components=80, background_rank=3, sim_iters=10)
    assert diag["max_components"] == 80 == ref.diag["max_components"]
    _check_full(pmd, diag, ref, mov)


def test_full_pipeline_max_components_80_every_component_kept(gpu_ctx):
    """The same with thresholds that every component passes: all 80 components of every tile are kept, so each tile spans
    two blocks of 64 component rows in the global stage (virtual tiles: Gram blocks between the two blocks of one tile,
    compaction, projection, CSR assembly with 80 columns per tile), first with R <= frames, then with R > frames."""
    mov = _movie(1000, 40, 50, seed=22)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (20, 20), 1000, max_components=80, background_rank=2, thresholds=(1e9, 1e9))
    assert np.all(diag["tile_ranks"] == 80) and np.all(ref.diag["tile_ranks"] == 80)
    assert pmd.u.shape[1] == 12 * 80 + 2 and diag["rank_before"] <= diag["crop"]
    # (every tile is cut at component 80 inside its cluster of noise-level singular values, so the span of a tile's kept
    # components is determined only up to that cluster: the last few of the 962 final components - s ~ 2e-3 s_1 - are
    # individually ill-determined on both sides; vt_tol scales the per-component bound eps s_1 / (s_c gap_c))
    _check_full(pmd, diag, ref, mov, vt_tol=2e-2)
    mov = _movie(900, 40, 70, seed=23)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (20, 20), 900, max_components=80, background_rank=2, thresholds=(1e9, 1e9))
    assert np.all(diag["tile_ranks"] == 80) and diag["rank_before"] > diag["crop"]
    _check_full(pmd, diag, ref, mov, vt_tol=2e-2, orth_tol=1e-2, s_tol=3e-3, vt_tol_signal=2e-3, probe_tol=5e-3)


def test_full_pipeline_background_rank_60(gpu_ctx):
    """background_rank = 60: a 70-column sketch of the standardised sample (pmd_loader.py:46-68), generic-width kernels in
    the background rSVD; 60 background columns in U, 60 background rows in the temporal matrix."""
    mov = _movie(800, 60, 60, seed=24)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (20, 20), 800, max_components=6, background_rank=60, sim_iters=10)
    assert pmd.u.shape[1] == int(diag["tile_ranks"].sum()) + 60
    _check_full(pmd, diag, ref, mov, vt_tol=3e-3)


def test_full_pipeline_background_rank_100(gpu_ctx):
    """background_rank above 64 (unbounded in the reference, pmd_loader.py:300-314): the filter, the projection and the
    background blocks of U^T U run in blocks of 64 background columns.  First with R <= frames (dense U^T U), then with
    R > frames (block-sparse U^T U with two background blocks per tile)."""
    mov = _movie(1000, 60, 60, seed=41)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (20, 20), 1000, max_components=6, background_rank=100, sim_iters=10)
    assert pmd.u.shape[1] == int(diag["tile_ranks"].sum()) + 100 and diag["rank_before"] <= diag["crop"]
    # (the comparison counts every background column as a "stable" column of U; with 70-100 of them the last ones are
    # noise-level singular vectors of the 1000-frame sample with gaps of a few per cent: u_tol 2e-3 instead of 5e-4)
    _check_full(pmd, diag, ref, mov, vt_tol=3e-3, u_tol=2e-3)
    mov = _movie(300, 70, 80, seed=42)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (10, 10), 300, max_components=8, background_rank=70, sim_iters=10)
    assert diag["rank_before"] > diag["crop"]
    _check_full(pmd, diag, ref, mov, vt_tol=5e-3, orth_tol=1e-2, s_tol=3e-3, vt_tol_signal=2e-3, probe_tol=5e-3, u_tol=2e-3)


def test_full_pipeline_tiles_above_2048_pixels(gpu_ctx):
    """48 x 50-pixel blocks (2400 pixels; the reference accepts any even block size >= 10, decomposition.py:572-613): the tile
    contractions split the pixel axis over the grid in slices of 1024 (three slices here), pooled tiles of 600 pixels."""
    mov = _movie(600, 96, 100, seed=43)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (48, 50), 600, max_components=8, background_rank=3, sim_iters=10)
    assert diag["dpad"] == 3072 and len(diag["tile_ranks"]) == 9
    _check_full(pmd, diag, ref, mov, vt_tol=3e-3)


def test_full_pipeline_subsampled_frames_and_no_background(gpu_ctx):
    mov = _movie(900, 36, 44, seed=2)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (16, 20), 300, max_components=5, background_rank=0, sim_iters=10)
    _check_full(pmd, diag, ref, mov)
    assert pmd.u.shape[1] == ref.u.shape[1]


def test_full_pipeline_rank_exceeds_frames(gpu_ctx):
    # many tiles, few frames: R > Tf exercises the right_mat = v branch (decomposition.py:976-977)
    mov = _movie(300, 70, 80, seed=3)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (10, 10), 300, max_components=8, background_rank=3, sim_iters=10)
    assert diag["rank_before"] > diag["crop"]
    # fp32 Gram-eigh limit of this branch: the oracle itself keeps a numerically-null direction here
    # (lambda ~ +1e-7 lambda_max) and reaches only |(UR)^T(UR) - I| ~ 1; the HIP path drops it.
    _check_full(pmd, diag, ref, mov, vt_tol=5e-3, orth_tol=1e-2, s_tol=3e-3, vt_tol_signal=2e-3)


def test_reference_test_suite_shapes(gpu_ctx):
    """/root/reference/test/test_pmd.py:30-61: rank-30 150x150x1000 data, blocks 32/28/40,
    frames_to_init 5000 > T, background_rank 1, max_components 40: must run to completion."""
    import localmd_amd
    from localmd_amd import decomposition as Dm

    Dm.QUIET = True
    rng = np.random.default_rng(0)
    spatial = rng.random((150, 150, 30))
    temporal = rng.random((30, 1000))
    data = np.tensordot(spatial, temporal, axes=(2, 0)).transpose(2, 0, 1)
    for blk in [(32, 32), (28, 40)]:
        np.random.seed(0)
        out = localmd_amd.localmd_decomposition(data, list(blk), 5000, max_components=40, background_rank=1, sim_conf=5,
                                                frame_batch_size=2000, pixel_batch_size=10000, dtype="float32",
                                                num_workers=0, max_consecutive_failures=1, rank_prune=False, ctx=gpu_ctx,
                                                sim_iters=10, seed=1)
        assert out.shape == (1000, 150, 150)
        assert np.all(np.isfinite(out.s)) and np.all(np.isfinite(out.v)) and np.all(np.isfinite(out.r))
        frame = out[10, :, :]
        assert frame.shape == (150, 150) and np.all(np.isfinite(frame))


def test_block_size_errors(gpu_ctx):
    import localmd_amd

    mov = _movie(120, 30, 30, seed=1)
    with pytest.raises(ValueError):
        localmd_amd.localmd_decomposition(mov, (8, 20), 100, ctx=gpu_ctx)
    with pytest.raises(ValueError):
        localmd_amd.localmd_decomposition(mov[:, :9, :], (20, 20), 100, ctx=gpu_ctx)
    with pytest.raises(ValueError):
        localmd_amd.localmd_decomposition(mov, (20, 20), 100, temporal_avg_factor=200, ctx=gpu_ctx, sim_iters=2)


def test_orthogonalizer_variants_agree(gpu_ctx):
    """R > frames: the Cholesky form of P and the reference's eigenvector form give the same R, s, Vt
    (they differ by an orthogonal factor absorbed by the projected SVD)."""
    import localmd_amd
    from localmd_amd import decomposition as Dm

    Dm.QUIET = True
    mov = _movie(300, 70, 80, seed=3)
    outs = {}
    for mode in ("eigh", "cholesky"):
        np.random.seed(7)
        outs[mode] = localmd_amd.localmd_decomposition(mov, (10, 10), 300, max_components=8, background_rank=3, sim_iters=10,
                                                       seed=123, orthogonalizer=mode, return_diagnostics=True, ctx=gpu_ctx)
    (a, da), (b, db) = outs["eigh"], outs["cholesky"]
    assert da["orthogonalizer"] == "eigh" and db["orthogonalizer"] == "cholesky"
    np.testing.assert_array_equal(da["tile_ranks"], db["tile_ranks"])
    np.testing.assert_array_equal(a.u.indices, b.u.indices)
    n = min(len(a.s), len(b.s))
    strong = a.s[:n] > 5e-2 * a.s[0]
    np.testing.assert_allclose(b.s[:n][strong], a.s[:n][strong], rtol=2e-3)
    ura, urb = a.u @ a.r, b.u @ b.r
    eb = urb.T @ urb - np.eye(urb.shape[1])
    if db["null_direction"].get("split_off"):
        # the kept numerically null direction (last component): its pivot is floored at the fp32 rounding level (as the
        # reference's fp32 eigenvalue would be), so its column of U R has norm <= 1, not 1
        assert -1.0 - 1e-6 <= eb[-1, -1] <= 1e-2
        eb[-1, -1] = 0.0
    assert np.abs(eb).max() < 1e-2
    rng = np.random.default_rng(0)
    pi, pt = rng.integers(0, 5600, 400), rng.integers(0, 300, 400)
    ra = np.einsum("pk,k,kp->p", ura[pi], a.s, a.v[:, pt])
    rb = np.einsum("pk,k,kp->p", urb[pi], b.s, b.v[:, pt])
    assert np.abs(ra - rb).max() < 2e-3 * np.abs(ra).max()


def test_full_pipeline_multi_window_residual(gpu_ctx):
    """window_chunks < frame_range: first window single_block_md, later windows fit the residual
    (decomposition.py:333-387, :471-515)."""
    mov = _movie(900, 40, 44, seed=6)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (20, 20), 600, max_components=8, background_rank=2, sim_iters=10,
                                   window_chunks=200)
    assert len(diag["frames"]) == 600
    exact, knife = _check_full(pmd, diag, ref, mov, vt_tol=3e-3)
    # the later windows must have contributed components in at least one tile
    first = np.array([d[0]["kept"].sum() for d in ref.diag["tile_diag"]])
    assert np.any(ref.diag["tile_ranks"] > first)


def test_full_pipeline_multi_window_residual_max_components_70(gpu_ctx):
    """Residual windows on the generic-width path (max_components + 10 > 64: 128 component rows per tile): the first window
    through the wide single_block_md, the second through the wide single_residual_block_md (decomposition.py:333-387), then
    the projection of the running basis over all fitted frames in blocks of 64 component rows."""
    mov = _movie(1700, 40, 44, seed=31)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (20, 20), 1600, max_components=70, background_rank=2, sim_iters=10,
                                   window_chunks=800)
    assert len(diag["frames"]) == 1600 and diag["max_components"] == 70
    _check_full(pmd, diag, ref, mov, vt_tol=3e-3)
    first = np.array([d[0]["kept"].sum() for d in ref.diag["tile_diag"]])
    assert np.any(ref.diag["tile_ranks"] > first)


def test_full_pipeline_max_components_beyond_time_bins(gpu_ctx):
    """max_components larger than frames / temporal_avg_factor: the reference's rSVD keeps its (max_components + 10)-column
    sketch and returns the components that exist (decomposition.py:59-73, `u_final[:, :rank]`); no error."""
    mov = _movie(300, 44, 40, seed=8)
    # (cut-offs injected between the statistics of signal and of noise components: with 30 bins per tile the simulated
    # ones sit inside the noise distribution and the decisions of the noise components become coin flips on both sides)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (22, 20), 300, max_components=40, background_rank=2, thresholds=(1.0, 1.7),
                                   temporal_avg_factor=10)
    assert diag["tile_ranks"].max() <= 30
    np.testing.assert_array_equal(diag["tile_ranks"], ref.diag["tile_ranks"])
    assert pmd.s.shape == ref.s.shape
    # Structure and fit, not the element-wise classes of _check_full: the standardised traces sum to zero, so the binned
    # tile has rank 29 and its 30th left vector is LAPACK's arbitrary completion in the reference and the zero vector here
    # (numerical policy); through V_ds that adds one arbitrary direction to the row space the final tile
    # SVD works in, which moves every later quantity by ~1e-3 on either side.
    assert pmd.u.shape == ref.u.shape and pmd.r.shape == ref.r.shape and pmd.v.shape == ref.v.shape
    np.testing.assert_array_equal(pmd.u.indptr, ref.u.indptr)
    np.testing.assert_array_equal(pmd.u.indices, ref.u.indices)
    assert np.all(np.isfinite(pmd.r)) and np.all(np.isfinite(pmd.v)) and np.all(np.isfinite(pmd.s))
    k = len(ref.s) // 4
    np.testing.assert_allclose(pmd.s[:k], ref.s[:k], rtol=5e-3)
    rng = np.random.default_rng(0)
    pi, pt = rng.integers(0, 44 * 40, 500), rng.integers(0, 300, 500)
    y = ((mov - ref.mean_img[None]) / ref.std_img[None]).reshape(300, -1, order="F")[pt, pi]
    fit = [float(np.mean((np.einsum("pk,k,kp->p", np.asarray(x.u.tocsr()[pi] @ x.r), x.s, x.v[:, pt]) - y) ** 2)) for x in (pmd, ref)]
    assert abs(fit[0] - fit[1]) < 0.02 * fit[1], fit


def test_full_pipeline_rank_prune(gpu_ctx):
    """rank_prune=True (decomposition.py:861-877): the right matrix is v_cropped times a Gaussian matrix
    (device stream PRUNE, handed to the oracle as is)."""
    mov = _movie(500, 40, 44, seed=5)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (20, 20), 500, max_components=6, background_rank=2, sim_iters=10,
                                   rank_prune=True, rank_prune_factor=0.5)
    assert pmd.s.shape == ref.s.shape
    _check_full(pmd, diag, ref, mov, vt_tol=5e-3, orth_tol=1e-2, s_tol=3e-3, vt_tol_signal=2e-3)


def test_full_pipeline_pixel_weighting_and_c_order(gpu_ctx):
    """pixel_weighting (decomposition.py:740-741) and order='C' (pmd_loader.py reshape order)."""
    mov = _movie(400, 36, 40, seed=6)
    rng = np.random.default_rng(3)
    pw = (0.5 + rng.random((36, 40))).astype(np.float32)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (18, 20), 400, max_components=5, background_rank=1, sim_iters=10,
                                   pixel_weighting=pw, order="C")
    # the weakest "signal" component of this case (sigma = 5.4 % of sigma_1, 2.7 % gap) sits at the fp32
    # Gram-eigh limit eps (sigma_1/sigma_c)^2 / gap ~ 8e-4 of BOTH implementations; all others are < 4e-5
    _check_full(pmd, diag, ref, mov, vt_tol_signal=6e-4)
    assert pmd.order == "C"


@pytest.mark.parametrize("case", [
    # (T, d1, d2, block, frame_range, kwargs)
    dict(T=777, d1=33, d2=41, block=(12, 14), frames=500, kw=dict(max_components=7, background_rank=3, temporal_avg_factor=5)),
    dict(T=1000, d1=48, d2=30, block=(16, 10), frames=1000, kw=dict(max_components=5, background_rank=1, spatial_avg_factor=1)),
    dict(T=640, d1=64, d2=64, block=(32, 32), frames=640, kw=dict(max_components=12, background_rank=4, temporal_avg_factor=8)),
    dict(T=450, d1=27, d2=52, block=(18, 26), frames=450, kw=dict(max_components=4, background_rank=0, max_consecutive_failures=2)),
    dict(T=1210, d1=30, d2=30, block=(10, 10), frames=300, kw=dict(max_components=9, background_rank=2, compute_normalizer=False)),
    dict(T=520, d1=44, d2=36, block=(22, 12), frames=520, kw=dict(max_components=6, background_rank=2, spatial_avg_factor=3,
                                                              temporal_avg_factor=4)),
    # R > frames with frames % temporal_avg_factor != 0: the traces are centred over all 303 frames but fitted on the first
    # 300, so the constant vector is no exact null direction and must not be deflated
    dict(T=303, d1=50, d2=50, block=(10, 10), frames=303, kw=dict(max_components=8, background_rank=2)),
    # the same with more tile components than frames (R = 1275 > 300: right-matrix route, Cholesky without deflation)
    dict(T=303, d1=70, d2=80, block=(10, 10), frames=303, kw=dict(max_components=8, background_rank=3)),
])
def test_full_pipeline_assorted_shapes(gpu_ctx, case):
    """Ragged sizes: FOV not a multiple of the block stride (snapped last tiles), odd frame counts, every
    averaging factor, no background, several allowed failures, no normaliser."""
    mov = _movie(case["T"], case["d1"], case["d2"], seed=case["T"])
    pmd, diag, ref = _compare_full(gpu_ctx, mov, case["block"], case["frames"], sim_iters=8, **case["kw"])
    use_right = diag["rank_before"] > diag["crop"]
    if use_right and case["T"] == 303:
        assert diag["crop"] == 300 and diag["rank_before"] > diag["crop"]
        _check_full(pmd, diag, ref, mov, vt_tol=5e-3, orth_tol=1e-2, s_tol=3e-3, vt_tol_signal=2e-3, probe_tol=6e-2)
    elif use_right:
        _check_full(pmd, diag, ref, mov, vt_tol=5e-3, orth_tol=1e-2, s_tol=3e-3, vt_tol_signal=2e-3)
    elif case["T"] == 303:
        # ten pixels per block side: the one failing component every tile keeps is an arbitrary vector of the tile's
        # noise subspace on either side, and with 81 such tiles on 50 x 50 pixels the reconstructions
        # differ by the noise those components carry (3.6 % of the peak, measured); everything well posed is compared
        _check_full(pmd, diag, ref, mov, vt_tol=3e-3, probe_tol=6e-2)
    else:
        _check_full(pmd, diag, ref, mov, vt_tol=3e-3)


def test_full_pipeline_long_time_axis(gpu_ctx):
    """T = 5000 frames (five Welch chunks, 500 temporal bins per tile, 157 time chunks in the tile GEMMs)."""
    mov = _movie(5000, 40, 40, seed=11)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (20, 20), 5000, max_components=8, background_rank=3, sim_iters=8)
    _check_full(pmd, diag, ref, mov, vt_tol=3e-3)


def _smooth_time(v):
    """(traces, frames) -> same shape; works on numpy arrays (oracle) and torch device tensors (HIP path)."""
    out = v * 1.0
    out[:, 1:-1] = 0.25 * v[:, :-2] + 0.5 * v[:, 1:-1] + 0.25 * v[:, 2:]
    return out


def _smooth_space(s):
    """(components, b1, b2) -> same shape: 5-point smoothing of the interior."""
    out = s * 1.0
    out[:, 1:-1, 1:-1] = 0.5 * s[:, 1:-1, 1:-1] + 0.125 * (s[:, :-2, 1:-1] + s[:, 2:, 1:-1] + s[:, 1:-1, :-2] + s[:, 1:-1, 2:])
    return out


@pytest.mark.parametrize("which", ["temporal", "spatial", "both"])
def test_full_pipeline_denoiser_hooks(gpu_ctx, which):
    """spatial_denoiser / temporal_denoiser of single_block_md (decomposition.py:300, :304-313).  The hooks are
    linear here, so the result does not depend on the sign / rotation conventions of the intermediate bases."""
    mov = _movie(600, 40, 50, seed=21)
    kw = dict(max_components=6, background_rank=2, sim_iters=10)
    if which in ("temporal", "both"):
        kw["temporal_denoiser"] = _smooth_time
    if which in ("spatial", "both"):
        kw["spatial_denoiser"] = _smooth_space
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (20, 20), 600, **kw)
    _check_full(pmd, diag, ref, mov, vt_tol=3e-3)
    # the hook changes the answer (guards against a silently ignored argument)
    plain, _, _ = _compare_full(gpu_ctx, mov, (20, 20), 600, max_components=6, background_rank=2, sim_iters=10)
    assert plain.u.shape != pmd.u.shape or not np.allclose(plain.u.data, pmd.u.data, rtol=1e-4, atol=1e-6)


def test_full_pipeline_denoiser_hooks_generic_width(gpu_ctx):
    """Both hooks on the generic-width tile path (max_components = 60: 128 component rows; the three resumable stages of
    pmd_tiles_decompose_staged with the hook arrays at their rp-row offsets)."""
    mov = _movie(900, 40, 50, seed=33)
    kw = dict(max_components=60, background_rank=2, sim_iters=10, temporal_denoiser=_smooth_time, spatial_denoiser=_smooth_space)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (20, 20), 900, **kw)
    assert diag["max_components"] == 60
    _check_full(pmd, diag, ref, mov, vt_tol=3e-3)


def test_denoiser_hooks_batched_and_first_window_only(gpu_ctx):
    """A callable marked ``batched`` sees all tiles at once and gives the same result as the per-tile calls; with
    several temporal windows the hooks act in the first window only (decomposition.py:476-488)."""
    import localmd_amd
    from localmd_amd import decomposition as Dm

    Dm.QUIET = True
    mov = _movie(800, 40, 40, seed=22)
    calls = {"t": 0, "s": 0}

    def t_one(v):
        calls["t"] += 1
        assert v.ndim == 2 and v.shape == (5, 400) and v.is_cuda
        return torch_tanh(v)

    def s_one(s):
        calls["s"] += 1
        assert s.shape == (5, 20, 20) and s.is_cuda
        return _smooth_space(s)

    def torch_tanh(v):
        import torch

        sc = v.abs().amax(dim=-1, keepdim=True) + 1e-6
        return torch.tanh(2.0 * v / sc) * sc

    def t_all(v):
        assert v.ndim == 3 and v.shape[1:] == (5, 400)
        return torch_tanh(v)

    t_all.batched = True

    def s_all(s):
        assert s.ndim == 4 and s.shape[1:] == (5, 20, 20)
        out = s * 1.0
        out[:, :, 1:-1, 1:-1] = 0.5 * s[:, :, 1:-1, 1:-1] + 0.125 * (s[:, :, :-2, 1:-1] + s[:, :, 2:, 1:-1] +
                                                                      s[:, :, 1:-1, :-2] + s[:, :, 1:-1, 2:])
        return out

    s_all.batched = True
    kw = dict(max_components=5, background_rank=2, window_chunks=400, seed=5, thresholds=(1.0, 1.0), ctx=gpu_ctx)
    np.random.seed(3)
    a = localmd_amd.localmd_decomposition(mov, (20, 20), 800, temporal_denoiser=t_one, spatial_denoiser=s_one, **kw)
    assert calls == {"t": 9, "s": 9}  # 3 x 3 tiles, first window only
    np.random.seed(3)
    b = localmd_amd.localmd_decomposition(mov, (20, 20), 800, temporal_denoiser=t_all, spatial_denoiser=s_all, **kw)
    np.testing.assert_array_equal(a.u.indices, b.u.indices)
    np.testing.assert_array_equal(a.u.data, b.u.data)
    np.testing.assert_array_equal(a.s, b.s)
    with pytest.raises(ValueError):
        localmd_amd.localmd_decomposition(mov, (20, 20), 800, temporal_denoiser=lambda v: v[:, :-1], **kw)
    with pytest.raises(TypeError):
        localmd_amd.localmd_decomposition(mov, (20, 20), 800, spatial_denoiser="median", **kw)


@pytest.mark.parametrize("order", ["F", "C"])
def test_pmdarray_device_expansion_matches_host(gpu_ctx, order):
    """PMDArray.to_device(): __getitem__ on the GPU returns what the reference's SciPy / NumPy expansion
    (pmdarray.py:132-171) returns, for every kind of key and both pixel orders."""
    import localmd_amd
    from localmd_amd import decomposition as Dm

    Dm.QUIET = True
    mov = _movie(600, 40, 50, seed=31)
    np.random.seed(1)
    pmd = localmd_amd.localmd_decomposition(mov, (20, 20), 600, max_components=6, background_rank=2, seed=9, sim_iters=8,
                                            ctx=gpu_ctx, order=order)
    keys = [
        (slice(None),), (5,), (slice(10, 300, 7),), ([3, 1, 599, 1],), (slice(0, 64), slice(4, 30), slice(7, 50)),
        (slice(None), 7, 9), (17, slice(None), slice(None)), (slice(100, 420), [1, 5, 9], [2, 2, 40]),
        (np.array([0, 7, 8]), slice(0, 40, 3), 11), (slice(0, 5), 3), (slice(None), slice(None), slice(None)),
        (slice(2, 2), slice(None), slice(None)),
    ]
    host = [pmd[k if len(k) > 1 else k[0]] for k in keys]
    pmd.to_device(ctx=gpu_ctx)
    try:
        for k, h in zip(keys, host):
            g = pmd[k if len(k) > 1 else k[0]]
            assert g.shape == h.shape and g.dtype == h.dtype == np.float32, (k, g.shape, h.shape)
            np.testing.assert_allclose(g, h, rtol=2e-5, atol=2e-5 * max(1.0, float(np.abs(h).max()) if h.size else 1.0))
        # an empty spatial selection is refused by the reference's reshape (pmdarray.py:165): same exception on the device path
        with pytest.raises(ValueError):
            pmd[3, 5:5, :]
    finally:
        pmd.to_host()
    assert pmd._dev is None
    np.testing.assert_array_equal(pmd[5], host[1])
    with pytest.raises(ValueError):
        pmd[3, 5:5, :]


@pytest.mark.parametrize("which", ["no_columns", "rank_zero", "no_entries"])
def test_pmdarray_device_expansion_without_columns_rank_or_entries(gpu_ctx, which):
    """A U without columns (found by tests/test_gpu_consumer_fuzz.py on a 23 x 37 field: pmd_csr_rows_spmm refused the
    null pointers of the empty device arrays), factors of rank 0, and a U whose columns hold no entry: pmd[...] after
    to_device() is the mean image in every frame, as on the host."""
    import scipy.sparse
    from localmd_amd.pmdarray import PMDArray
    from tests.util import degenerate_pmds

    T, d1, d2 = 12, 5, 7
    rng = np.random.default_rng(3)
    f32 = np.float32
    full = PMDArray(scipy.sparse.random(d1 * d2, 4, density=0.4, random_state=1, format="csr", dtype=f32),
                    rng.standard_normal((4, 2)).astype(f32), np.ones(2, f32), rng.standard_normal((2, T)).astype(f32), (T, d1, d2),
                    "F", rng.uniform(500, 1500, (d1, d2)).astype(f32), rng.uniform(2, 10, (d1, d2)).astype(f32))
    if which == "no_entries":
        pmd = PMDArray(scipy.sparse.csr_matrix((d1 * d2, 4), dtype=f32), full.r, full.s, full.v, (T, d1, d2), "F", full.mean_img,
                       full.var_img)
    else:
        pmd = degenerate_pmds(full)[which]
    keys = [slice(None), 5, (slice(2, 9), slice(1, 4), slice(0, 7, 2)), ([3, 1, 11], 2, 6)]
    host = [pmd[k] for k in keys]
    assert np.array_equal(host[1], pmd.mean_img)
    pmd.to_device(ctx=gpu_ctx)
    try:
        for k, h in zip(keys, host):
            g = pmd[k]
            assert g.shape == h.shape and g.dtype == h.dtype == np.float32 and np.array_equal(g, h), k
    finally:
        pmd.to_host()


def _check_structure_and_fit(pmd, diag, ref, mov):
    """For inputs whose kept noise component is an arbitrary vector of a nearly degenerate noise subspace (very short
    movies): everything that is well posed - tile ranks, CSR structure, statistics images, orthonormality, and how
    well each side reconstructs the standardised movie on random probes."""
    T, d1, d2 = mov.shape
    np.testing.assert_array_equal(diag["tile_ranks"], ref.diag["tile_ranks"])
    np.testing.assert_array_equal(pmd.u.indptr, ref.u.indptr)
    np.testing.assert_array_equal(pmd.u.indices, ref.u.indices)
    np.testing.assert_allclose(pmd.mean_img, ref.mean_img, rtol=1e-5)
    np.testing.assert_allclose(pmd.var_img, ref.std_img, rtol=2e-4)
    ur, ur_ref = pmd.u @ pmd.r, ref.u @ ref.r
    assert np.abs(ur.T @ ur - np.eye(ur.shape[1])).max() < 2e-3
    assert np.abs(pmd.v @ pmd.v.T - np.eye(pmd.v.shape[0])).max() < 2e-3
    n = min(len(pmd.s), len(ref.s))
    np.testing.assert_allclose(pmd.s[:2], ref.s[:2], rtol=2e-3)   # the signal part of the spectrum
    rng = np.random.default_rng(0)
    pi = rng.integers(0, d1 * d2, 600)
    pt = rng.integers(0, T, 600)
    y = ((mov - ref.mean_img[None]) / ref.std_img[None]).reshape(T, -1, order="F")[pt, pi]
    rec = np.einsum("pk,k,kp->p", ur[pi], pmd.s, pmd.v[:, pt])
    rec_ref = np.einsum("pk,k,kp->p", ur_ref[pi], ref.s, ref.v[:, pt])
    e_hip, e_ref = np.mean((rec - y) ** 2), np.mean((rec_ref - y) ** 2)
    assert abs(e_hip - e_ref) < 0.1 * e_ref + 1e-6, (e_hip, e_ref)
    return n


def test_full_pipeline_short_movie_and_single_tile(gpu_ctx):
    """Edge cases of the reference's argument handling: fewer than 256 frames (no Welch chunk: the noise image is
    all ones, pmd_loader.py:213-226), max_components larger than frames // temporal_avg_factor (capped with a
    warning, decomposition.py:764-770), a field of view that is exactly one tile, and temporal_avg_factor >= frames
    (ValueError, :762)."""
    import localmd_amd

    # With 20 temporal bins per tile the noise components (nearly equal singular values: their vectors are an arbitrary
    # rotation of the noise subspace in either implementation) have roughness statistics that straddle simulated
    # thresholds; injected thresholds between the signal and the noise statistics keep the rank decisions well posed.
    thr = (1.35, 1.8)
    mov = _movie(200, 20, 24, seed=41)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (10, 12), 200, max_components=50, background_rank=1, thresholds=thr)
    assert diag["max_components"] == 20 and np.all(pmd.var_img == 1.0)
    _check_structure_and_fit(pmd, diag, ref, mov)
    one = _movie(300, 10, 12, seed=42)
    pmd1, diag1, ref1 = _compare_full(gpu_ctx, one, (10, 12), 300, max_components=4, background_rank=0, thresholds=thr)
    assert len(diag1["tile_ranks"]) == 1
    _check_structure_and_fit(pmd1, diag1, ref1, one)
    with pytest.raises(ValueError):
        localmd_amd.localmd_decomposition(mov, (10, 12), 200, temporal_avg_factor=200, ctx=gpu_ctx, seed=1,
                                          thresholds=(1.0, 1.0))


@pytest.mark.parametrize("case", [
    dict(T=500, d1=40, d2=40, block=(20, 20), frames=500, kw=dict(max_components=1, background_rank=2)),
    dict(T=600, d1=30, d2=36, block=(10, 12), frames=600, kw=dict(max_components=5, background_rank=20)),
    dict(T=300, d1=40, d2=30, block=(20, 10), frames=300, kw=dict(max_components=6, background_rank=2, temporal_avg_factor=1,
                                                                spatial_avg_factor=1)),
    dict(T=400, d1=88, d2=66, block=(44, 44), frames=400, kw=dict(max_components=10, background_rank=3)),
    dict(T=512, d1=30, d2=100, block=(20, 40), frames=512, kw=dict(max_components=7, background_rank=1, max_consecutive_failures=3)),
])
def test_full_pipeline_extreme_arguments(gpu_ctx, case):
    """One component per tile, a background rank larger than the tile ranks, no averaging at all, the largest tile
    variant (1936 pixels), an elongated field of view with blocks larger than half of it."""
    mov = _movie(case["T"], case["d1"], case["d2"], seed=case["T"] + case["d1"])
    pmd, diag, ref = _compare_full(gpu_ctx, mov, case["block"], case["frames"], sim_iters=8, **case["kw"])
    use_right = diag["rank_before"] > diag["crop"]
    if case["kw"].get("max_consecutive_failures", 1) >= 3:
        # three failing components are kept per tile: vectors of the (nearly degenerate) noise subspace, arbitrary in
        # either implementation, so the probes of the reconstruction agree only to the noise they carry (0.5 % here)
        _check_structure_and_fit(pmd, diag, ref, mov)
    elif use_right:
        _check_full(pmd, diag, ref, mov, vt_tol=5e-3, orth_tol=1e-2, s_tol=3e-3, vt_tol_signal=2e-3)
    else:
        _check_full(pmd, diag, ref, mov, vt_tol=3e-3)


def test_tiff_dataset_end_to_end(gpu_ctx, tmp_path):
    """The dataset contract (dataset.py:38-114: shape + obj[list of frames]) through the TIFF reader: a uint16
    multipage file decomposes to exactly what the same frames give as an in-memory array, in small frame batches."""
    import localmd_amd
    from localmd_amd import decomposition as Dm
    from localmd_amd._minitiff import write_tiff

    Dm.QUIET = True
    mov = np.clip(_movie(420, 40, 30, seed=51) * 4.0 + 200.0, 0, 65535).astype(np.uint16)
    fn = str(tmp_path / "movie.tif")
    write_tiff(fn, mov)
    kw = dict(max_components=5, background_rank=2, seed=3, thresholds=(1.2, 1.9), ctx=gpu_ctx)
    np.random.seed(5)
    a = localmd_amd.localmd_decomposition(localmd_amd.TiffArray(fn), (20, 10), 420, frame_batch_size=64, **kw)
    np.random.seed(5)
    b = localmd_amd.localmd_decomposition(mov.astype(np.float32), (20, 10), 420, **kw)
    np.testing.assert_array_equal(a.u.indices, b.u.indices)
    np.testing.assert_array_equal(a.u.data, b.u.data)
    np.testing.assert_array_equal(a.s, b.s)
    np.testing.assert_array_equal(a.v, b.v)
    np.testing.assert_array_equal(a.mean_img, b.mean_img)
    assert a.shape == (420, 40, 30) and a[7].shape == (40, 30)


def test_tiff_fixture_from_an_independent_writer_end_to_end(gpu_ctx):
    """SURVEY 8(f)1 with a file this repository did not write: tests/golden/pillow_u16_movie_deflate.tif (Pillow /
    libtiff, deflate-compressed, 260 pages; tests/golden/make_tiff_fixtures.py).  Decomposing it through TiffArray
    gives exactly what the pixel values stored next to it give as an in-memory array, and the oracle agrees on the
    structure of that result."""
    import os
    import localmd_amd
    from localmd_amd import decomposition as Dm

    Dm.QUIET = True
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    mov = np.load(os.path.join(golden, "tiff_fixture_expected.npz"))["movie"]
    kw = dict(max_components=5, background_rank=2, seed=3, thresholds=(1.2, 1.9), ctx=gpu_ctx)
    np.random.seed(5)
    a, diag = localmd_amd.localmd_decomposition(localmd_amd.TiffArray(os.path.join(golden, "pillow_u16_movie_deflate.tif")),
                                                (16, 12), 260, frame_batch_size=50, return_diagnostics=True, **kw)
    np.random.seed(5)
    b = localmd_amd.localmd_decomposition(mov.astype(np.float32), (16, 12), 260, **kw)
    np.testing.assert_array_equal(a.u.indices, b.u.indices)
    np.testing.assert_array_equal(a.u.data, b.u.data)
    np.testing.assert_array_equal(a.s, b.s)
    np.testing.assert_array_equal(a.v, b.v)
    np.testing.assert_array_equal(a.mean_img, b.mean_img)
    np.random.seed(5)
    ref = O.localmd_decomposition(mov.astype(np.float32), (16, 12), 260, max_components=5, background_rank=2,
                                  rng=DeviceSource(gpu_ctx, 3), thresholds=(1.2, 1.9))
    np.testing.assert_array_equal(diag["tile_ranks"], ref.diag["tile_ranks"])
    np.testing.assert_array_equal(a.u.indptr, ref.u.indptr)
    np.testing.assert_array_equal(a.u.indices, ref.u.indices)
    np.testing.assert_allclose(a.mean_img, ref.mean_img, rtol=1e-5, atol=1e-3)


def test_public_svd_helpers_match_oracle():
    """localmd_amd.projected_svd / compute_lowrank_factorized_svd (the reference's two other public entry points,
    decomposition.py:936-1060) on the device against the oracle: both branches of each."""
    import scipy.sparse
    import localmd_amd

    rng = np.random.default_rng(4)
    # projected_svd: fewer rows than columns, then fewer columns than rows
    p = np.linalg.qr(rng.standard_normal((40, 12)))[0].astype(np.float32)
    v = (rng.standard_normal((12, 90)) * np.linspace(10, 1, 12)[:, None]).astype(np.float32)
    for pp, vv in ((p, v), (rng.standard_normal((7, 90)).astype(np.float32), v.T.copy())):
        r, s, vt = localmd_amd.projected_svd(pp, vv)
        r0, s0, vt0 = O.projected_svd(pp, vv)
        assert r.shape == r0.shape and s.shape == s0.shape and vt.shape == vt0.shape
        np.testing.assert_allclose(s, s0, rtol=2e-4, atol=2e-4 * s0.max())
        np.testing.assert_allclose((r * s) @ vt, pp @ vv, atol=1e-3 * np.abs(pp @ vv).max())
        k = min(6, len(s0))
        va = sign_align(vt[:k], vt0[:k], axis=1)
        assert np.abs(va - vt0[:k]).max() < 2e-3
    # compute_lowrank_factorized_svd: R <= frames (identity right matrix) and R > frames (right matrix = v)
    u = scipy.sparse.random(300, 20, density=0.2, random_state=1, format="coo")
    for ncol in (50, 8):
        vm = rng.standard_normal((20, ncol)).astype(np.float32)
        pl = localmd_amd.compute_lowrank_factorized_svd(u, vm, only_left=True)
        p0 = O.compute_lowrank_factorized_svd(u, vm, only_left=True)
        assert pl.shape == p0.shape
        up = u @ pl
        assert np.abs(up.T @ up - np.eye(pl.shape[1])).max() < 2e-3
        rr, ss, vvt = localmd_amd.compute_lowrank_factorized_svd(u, vm, only_left=False)
        r0, s0, vt0 = O.compute_lowrank_factorized_svd(u, vm, only_left=False)
        np.testing.assert_allclose(ss, s0, rtol=5e-4, atol=5e-4 * s0.max())
        full, full0 = (u @ rr) * ss @ vvt, (u @ r0) * s0 @ vt0
        np.testing.assert_allclose(full, full0, atol=2e-3 * np.abs(full0).max())


@pytest.mark.parametrize("case", [
    dict(T=600, d1=40, d2=50, block=(20, 20), frames=600, kw=dict(max_components=6, background_rank=2)),
    dict(T=900, d1=36, d2=44, block=(16, 20), frames=300, kw=dict(max_components=5, background_rank=0)),
    dict(T=640, d1=64, d2=64, block=(32, 32), frames=640, kw=dict(max_components=12, background_rank=4, temporal_avg_factor=8)),
])
def test_full_pipeline_against_single_precision_lapack_oracle(gpu_ctx, case, monkeypatch):
    """The same comparison with the oracle's QR / SVD / eigh in true single precision (scipy.linalg s-routines, the
    precision of jaxlib's CPU kernels for the reference's float32 arrays) instead of numpy.linalg's double: the
    tolerances of the default comparison still hold."""
    monkeypatch.setattr(O, "LAPACK_PRECISION", "single")
    mov = _movie(case["T"], case["d1"], case["d2"], seed=case["T"] // 3)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, case["block"], case["frames"], sim_iters=8, **case["kw"])
    _check_full(pmd, diag, ref, mov, vt_tol=3e-3)


def test_tile_batches_and_single_copy_plan_match_the_default_path(gpu_ctx):
    """The memory plan for movies that fill the HBM (BASELINE configs 4 / 5): tiles fitted and projected in batches
    (`tile_batch_bytes`), one standardised copy with the rank-K correction of the projection (`single_copy`).  Batching
    must not change a bit of the tile results; the single-copy projection agrees to fp32 rounding.  Both routes of the
    global stage (R <= frames, R > frames)."""
    import localmd_amd
    from localmd_amd import decomposition as Dm

    Dm.QUIET = True
    for mov, blk, kw in [(_movie(500, 60, 70, seed=4), (20, 20), dict(max_components=6, background_rank=3)),
                         (_movie(300, 70, 80, seed=3), (10, 10), dict(max_components=8, background_rank=3))]:
        outs = []
        for extra in (dict(), dict(tile_batch_bytes=1), dict(tile_batch_bytes=1, single_copy=True), dict(single_copy=True)):
            np.random.seed(7)
            outs.append(localmd_amd.localmd_decomposition(mov, blk, mov.shape[0], seed=11, sim_iters=8, return_diagnostics=True,
                                                          ctx=gpu_ctx, **kw, **extra))
        (a, da), (b, db), (c, dc), (e, de) = outs
        # batches of 64 tiles: same tile results bit for bit, same final result
        np.testing.assert_array_equal(da["tile_ranks"], db["tile_ranks"])
        np.testing.assert_array_equal(da["tile_ut"], db["tile_ut"])
        np.testing.assert_array_equal(a.u.data, b.u.data)
        np.testing.assert_allclose(b.s, a.s, rtol=1e-6)
        for x in (c, e):
            np.testing.assert_array_equal(x.u.indices, a.u.indices)
            np.testing.assert_array_equal(x.u.data, a.u.data)
            assert x.s.shape == a.s.shape
            # the projection differs by fp32 rounding ((X - B Pj) + B Pj against X); a singular value carries that
            # rounding times (s_1 / s_c)^2, like every quantity of the Gram-based final SVD
            tol = np.maximum(2e-5, 2e-6 * (a.s[0] / a.s) ** 2)
            strong = a.s > 1e-2 * a.s[0]
            assert np.all((np.abs(x.s - a.s) / a.s)[strong] <= tol[strong]), np.max((np.abs(x.s - a.s) / a.s / tol)[strong])
            assert PM.probes(x, a, mov.shape, n=400) < 2e-4


# Constant content: (what is overwritten, background_rank, further arguments).  The values are integers c with T c < 2^24.
_CONSTANT_KINDS = {
    "dead pixels": (("pixels",), 0, {}),
    "dead row": (("row",), 2, {}),
    "interior constant tile": (("tile",), 0, {}),
    "saturated block": (("saturated",), 2, {}),
    "zero pixel": (("zero pixel",), 0, {"compute_normalizer": False}),
    "dead column + pixels": (("column", "pixels"), 2, {}),
    "half dead": (("half",), 0, {}),
    "constant border band": (("band",), 2, {}),
    "interior constant tile, residual windows": (("tile",), 2, {"window_chunks": 160}),
    "dead row, max_components 60": (("row",), 0, {"max_components": 60}),
}


def _constant_movie(what, trial):
    """(movie (T, 40, 50), mask of the constant pixels, their values)."""
    T, d1, d2 = 320, 40, 50
    mov = _movie(T, d1, d2, seed=70 + trial)
    value = np.full((d1, d2), np.nan, dtype=np.float32)
    rng = np.random.default_rng(trial)
    if "pixels" in what:
        idx = rng.integers(0, d1 * d2, 12)
        value.reshape(-1)[idx] = 100.0
    if "row" in what:
        value[d1 // 2, :] = 7.0
    if "column" in what:
        value[:, 3] = 55.0
    if "tile" in what:
        value[:22, :22] = 100.0
    if "saturated" in what:
        value[5:15, 8:20] = 4095.0
    if "zero pixel" in what:
        value[4, 4] = 0.0
    if "half" in what:
        value[:, :d2 // 2] = 1.0
    if "band" in what:
        value[:3, :] = value[-3:, :] = value[:, :3] = value[:, -3:] = 17.0
    mask = ~np.isnan(value)
    mov[:, mask] = value[mask]
    assert float(np.nanmax(value)) * T < 2 ** 24
    return mov, mask, value


@pytest.mark.parametrize("kind", list(_CONSTANT_KINDS))
def test_full_pipeline_constant_pixels_rows_and_tiles(gpu_ctx, kind):
    """Movies with dead and saturated pixels, dead rows and columns, a constant half, an all-constant tile and a constant
    border band on all four sides (what register_movie(border=<constant>) and register_piecewise leave), through the
    driver against the oracle: what INTEGRATION.md ("All-constant tiles") promises.  One kind runs with residual windows
    (pmd_tiles_residual on a constant tile), one at the generic width (max_components = 60).

    The statistics images within the tolerances of the other parity tests; every factor finite on both sides; tile ranks
    equal (an all-constant tile keeps one failing component per window, as in the reference); the oracle never has fewer
    singular values, at most one more per kept component of an all-constant tile - such a component is a zero vector
    here, an arbitrary unit vector with a zero trace there - and those are below 1e-5 s_1; the fit of the standardised
    movie on random probes within 3 % + 1e-6 of the oracle's.  Measured on MI355X: one all-constant tile 46 / 46
    components, three (half dead) 26 / 26, one fitted in two windows 45 / 47 with the oracle's extra values at 1.0e-8 s_1
    and 8.3e-9 s_1; no difference in the kinds without an all-constant tile.

    A constant pixel with an integer value c, T c < 2^24: the fp32 mean is exact, the standardised trace exactly zero, and
    pmd[:, i, j] equals c bit for bit, expanded on the host and after to_device()."""
    from localmd_amd import grid
    from tests.test_gpu_fuzz import probe_fit

    what, bg, extra_kw = _CONSTANT_KINDS[kind]
    trial = list(_CONSTANT_KINDS).index(kind)
    mov, mask, value = _constant_movie(what, trial)
    T, d1, d2 = mov.shape
    kw = dict(max_components=5, background_rank=bg, thresholds=(1.0, 1.7))
    kw.update(extra_kw)
    pmd, diag, ref = _compare_full(gpu_ctx, mov, (20, 20), T, **kw)
    np.testing.assert_allclose(pmd.mean_img, ref.mean_img, rtol=1e-5)
    np.testing.assert_allclose(pmd.var_img, ref.std_img, rtol=2e-4)
    for res in (pmd, ref):
        assert all(np.all(np.isfinite(x)) for x in (res.s, res.r, res.v, res.u.data)), kind
    it1, it2 = grid.tile_origins((d1, d2), (20, 20))
    constant = np.array([bool(mask[k:k + 20, j:j + 20].all()) for k in it1 for j in it2])
    n_constant, n_null = int(constant.sum()), int(diag["tile_ranks"][constant].sum())
    extra = len(ref.s) - len(pmd.s)
    fit = (probe_fit(pmd, mov, ref.mean_img, ref.std_img, "F"), probe_fit(ref, mov, ref.mean_img, ref.std_img, "F"))
    print(f"\n{kind}: tile ranks {diag['tile_ranks'].tolist()} / {ref.diag['tile_ranks'].tolist()}, all-constant tiles {n_constant}, "
          f"their kept components {n_null}, components {len(pmd.s)} / {len(ref.s)}, oracle's extra s / s_1 {(ref.s[len(pmd.s):] / ref.s[0]).tolist()}, fit {fit[0]:.5f} / {fit[1]:.5f}")
    np.testing.assert_array_equal(diag["tile_ranks"], ref.diag["tile_ranks"])
    assert ("tile" in what or "half" in what) == (n_constant > 0)
    assert 0 <= extra <= n_null, (kind, extra, n_constant, n_null)
    assert np.all(ref.s[len(pmd.s):] < 1e-5 * ref.s[0]), ref.s[len(pmd.s):]
    assert abs(fit[0] - fit[1]) < 0.03 * fit[1] + 1e-6, fit
    expected = np.broadcast_to(value[mask], (T, int(mask.sum())))
    host = pmd[:][:, mask]
    assert host.dtype == np.float32 and np.array_equal(host, expected), (kind, "host", float(np.abs(host - expected).max()))
    pmd.to_device(ctx=gpu_ctx)
    try:
        got = pmd[:][:, mask]
    finally:
        pmd.to_host()
    assert got.dtype == np.float32 and np.array_equal(got, expected), (kind, "device", float(np.abs(got - expected).max()))
