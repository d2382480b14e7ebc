"""
The movie-preparation stage entry point by entry point (GPU): pmd_stats, pmd_standardize_transpose, pmd_bg_project,
pmd_bg_filter, pmd_scale_rows, pmd_background_rsvd and pmd_threshold_sim called by name through the C ABI, each against the
plain float64 reference of the same operation (tests/prep_ref.py), at the sizes where the code switches: the Welch chunk
and window counts, the 64-pixel and 1024-pixel blocks, 16 / 17 and 64 / 65 basis columns, the generic-width kernels from
background rank 55 on, and the second batch of the simulation.

Every test fills its outputs with NaN and the context's workspace with 0xFF before the call, gives the output arrays
sentinel rows beyond the last pixel that must come back untouched, and asserts exact zeros where the contract promises zeros.
Every tolerance is a derived bound, a stated multiple of the fp32 oracle's own distance to the float64 reference, or the
ceiling the suite already had; each test prints the figure it measured before it asserts.
"""
import functools

import numpy as np
import pytest

from localmd_amd.synthetic import make_movie
from oracle import pmd_oracle as O, philox
from tests import prep_ref as R
from tests.util import DeviceSource

pytestmark = pytest.mark.gpu

PMD_ERR_ARG = -2
EPS = 2.0 ** -24      # half an ulp of fp32, relative
SENTINELS = 3         # rows beyond D in every output array


def _t():
    import torch

    return torch


def P(t):
    from localmd_amd._lib import ptr

    return ptr(t)


def _dev(ctx, a, dtype=None):
    return _t().from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ctx.device)


def _nan(ctx, *shape):
    return _t().full(shape, float("nan"), dtype=_t().float32, device=ctx.device)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _workspace(ctx, nbytes):
    ws = ctx.workspace(nbytes)
    ws.fill_(0xFF)
    return ws


def _padded(ctx, a, rows, ld, fill=0.0):
    """a (D, n) on the device in a rows x ld array, `fill` everywhere else."""
    x = _t().full((rows, ld), fill, dtype=_t().float32, device=ctx.device)
    x[:a.shape[0], :a.shape[1]] = _dev(ctx, a, np.float32)
    return x


def _untouched(t):
    return bool(_t().isnan(t).all().item())


def _orthonormal(rng, D, K):
    return np.linalg.qr(rng.standard_normal((D, K)))[0].astype(np.float32)


# ---------------------------------------------------------------------------------------------- pmd_stats
FOV = {117: (9, 13), 1: (1, 1), 64: (8, 8), 65: (5, 13)}
# The suite's ceiling for sigma was 2e-4 relative (against the fp32 oracle).  Measured on an MI355X against float64: at most
# 2.02e-7 over all cases of test_stats, a thousand times below; the assert is four times the measured value (the factor
# allows for other seeds and the rounding of another FFT order).
SIGMA_RTOL = 4 * 2.02e-7


@functools.lru_cache(maxsize=None)
def _stats_movie(kind, T, D):
    d1, d2 = FOV[D]
    mov = make_movie(T, d1, d2, seed=3).reshape(T, D)
    if kind == "camera":         # 16-bit camera regime: integers around 30000
        mov = np.round(mov + np.float32(30000.0)).astype(np.float32)
    elif kind == "constant":
        mov = mov.copy()
        mov[:, 40] = np.float32(517.25)
    mov.setflags(write=False)
    return mov


def _run_stats(ctx, mov, frame_const, normalizer):
    T, D = mov.shape
    md = _dev(ctx, mov.copy())      # (the cached movie is read-only)
    mean, std = _nan(ctx, D + SENTINELS), _nan(ctx, D + SENTINELS)
    ws = _workspace(ctx, ctx.lib.pmd_stats_workspace_bytes(T, D, frame_const))
    ctx.call("pmd_stats", P(md), T, D, frame_const, 1 if normalizer else 0, P(mean), P(std), P(ws), ws.numel())
    ctx.sync()
    assert _untouched(mean[D:]) and _untouched(std[D:])
    return mean[:D].cpu().numpy(), std[:D].cpu().numpy()


STATS_CASES = ([("plain", T, 117, 1024, True) for T in (255, 256, 257, 383, 384, 1024, 1279, 1280, 2100)] +
               [("plain", 700, 117, 1024, False)] +
               [("plain", 1300, D, 1024, True) for D in (1, 64, 65)] +
               [("camera", 1300, 117, 1024, True), ("constant", 1300, 117, 1024, True), ("plain", 1300, 117, 512, True)])


@pytest.mark.parametrize("kind,T,D,frame_const,normalizer", STATS_CASES,
                         ids=[f"{k}-T{T}-D{D}-fc{fc}-{'on' if nz else 'off'}" for k, T, D, fc, nz in STATS_CASES])
def test_stats(gpu_ctx, kind, T, D, frame_const, normalizer):
    """Mean: |got - ref| <= 16 2^-24 max_t |y| per pixel: the kernel adds 16-term fp32 partial sums (15 roundings of at most
    2^-24 * 16 max|y| each, over T / 16 partials, divided by T), adds the partials and the chunk tail in double, and rounds
    the mean once.  Sigma: relative distance to float64 at most SIGMA_RTOL.  Lengths around 256 and 384 move the window
    count, 1279 / 1280 the count of chunks that enter the average, frame_const = 512 the chunk length itself (three counted
    chunks, the last of 276 frames).
    Measured on an MI355X: mean error at most 1.39 2^-24 max|y| (T = 256); sigma within 2.02e-7 relative (T = 383; 1.2e-7
    to 2.0e-7 in every case with an estimate, 3.9e-8 for the single pixel), exactly 1 where no estimate is made."""
    mov = _stats_movie(kind, T, D)
    mean, std = _run_stats(gpu_ctx, mov, frame_const, normalizer)
    mean_ref, std_ref = R.stats_ref(mov, frame_const, normalizer)
    e_mean = np.abs(mean - mean_ref) / np.abs(mov).max(axis=0)
    e_std = np.abs(std - std_ref) / std_ref
    print(f"\nstats {kind} T={T} D={D} fc={frame_const}: mean err / max|y| = {e_mean.max() / EPS:.3g} x 2^-24, "
          f"sigma rel = {e_std.max():.3g}")
    assert np.all(e_mean <= 16 * EPS)
    if T < 256 or not normalizer:
        assert np.all(std == 1.0)
    else:
        assert np.all(e_std <= SIGMA_RTOL)
    if kind == "constant":
        assert std[40] == 1.0 and mean[40] == np.float32(517.25)
        assert np.all(np.delete(std, 40) != 1.0)


def test_stats_rejects_a_chunk_length_below_one(gpu_ctx):
    """Every chunk length >= 1 is honoured (test_stats runs 512 next to 1024); zero and negative ones are refused before
    anything is launched, and size no workspace."""
    ctx = gpu_ctx
    mov = _stats_movie("plain", 256, 117)
    md = _dev(ctx, mov.copy())
    mean, std = _nan(ctx, 117), _nan(ctx, 117)
    ws = _workspace(ctx, ctx.lib.pmd_stats_workspace_bytes(256, 117, 1024))
    for fc in (0, -1024):
        assert ctx.lib.pmd_stats_workspace_bytes(256, 117, fc) == 0
        rc = ctx.lib.pmd_stats(ctx.handle, P(md), 256, 117, fc, 1, P(mean), P(std), P(ws), ws.numel())
        assert rc == PMD_ERR_ARG
    ctx.sync()
    assert _untouched(mean) and _untouched(std)


# ---------------------------------------------------------------------------------------------- pmd_standardize_transpose
@pytest.mark.parametrize("listed", [True, False], ids=["frame-list", "frames-null"])
@pytest.mark.parametrize("D,nf", [(117, 120), (64, 64), (65, 65), (1, 3), (200, 257)])
def test_standardize_transpose(gpu_ctx, D, nf, listed):
    """A subtraction and a division of exact fp32 inputs, each correctly rounded (the library is built without fast-math):
    relative distance to float64 at most 3 2^-24 with no absolute term, and the bits of NumPy's fp32 (y - mu) / sd.  Columns
    [nf, ld) are exact zeros.  The frames-null cases run with a leading dimension above pmd_time_ld(nf).
    Measured on an MI355X: at most 0.997 2^-24 relative, and bit equality holds in every case."""
    ctx = gpu_ctx
    rng = np.random.default_rng(100 * D + nf)
    T = nf + 37
    mov = (100.0 + 3.0 * rng.standard_normal((T, D))).astype(np.float32)
    mu = mov.mean(axis=0).astype(np.float32)
    sd = (mov.std(axis=0) + 0.5).astype(np.float32)
    frames = np.sort(rng.choice(T, size=nf, replace=False)).astype(np.int32) if listed else np.arange(nf, dtype=np.int32)
    ld = ctx.lib.pmd_time_ld(nf) + (0 if listed else 68)
    out = _nan(ctx, D + SENTINELS, ld)
    md, mud, sdd = _dev(ctx, mov), _dev(ctx, mu), _dev(ctx, sd)
    fr = _dev(ctx, frames) if listed else None
    ctx.call("pmd_standardize_transpose", P(md), D, P(fr), nf, P(mud), P(sdd), P(out), ld)
    ctx.sync()
    assert _untouched(out[D:])
    got = out[:D].cpu().numpy()
    assert np.all(_bits(got[:, nf:]) == 0)
    ref = R.standardize_ref(mov[frames], mu, sd)
    err = np.abs(got[:, :nf] - ref)
    print(f"\nstandardize D={D} nf={nf}: rel = {(err / np.maximum(np.abs(ref), 1e-300)).max() / EPS:.3g} x 2^-24")
    assert np.all(err <= 3 * EPS * np.abs(ref))
    f32 = ((mov[frames] - mu[None, :]) / sd[None, :]).T
    assert np.array_equal(_bits(got[:, :nf]), _bits(f32))


# ---------------------------------------------------------------------------------------------- pmd_bg_project
# (D, T, K): max |got - ref| / max |ref| measured on an MI355X.  The suite's ceiling is 2e-4; every case lies more than ten
# times below it, so the assert is four times the measured value.
PROJECT_MEASURED = {(360, 120, 3): 2.23e-7, (1024, 64, 16): 2.90e-7, (1025, 65, 17): 4.60e-7, (2500, 130, 64): 5.08e-7,
                    (2500, 130, 65): 5.00e-7}
PROJECT_TOL = {case: min(2e-4, 4 * measured) for case, measured in PROJECT_MEASURED.items()}


@pytest.mark.parametrize("D,T,K", sorted(PROJECT_TOL))
def test_bg_project(gpu_ctx, D, T, K):
    """B^T X across the 1024-pixel block (1024 / 1025 / 2500 pixels), the one-row-tile launch at <= 16 columns (16 / 17) and
    the second pass of 64 columns (64 / 65).  xs has round_up(D, 1024) rows, zero from D on, as the header asks; the basis
    has orthonormal columns; the projections are written with a leading dimension of their own.
    Tolerance: max |got - ref| <= PROJECT_TOL max |ref|.  Measured on an MI355X (PROJECT_MEASURED): 2.23e-7, 2.90e-7, 4.60e-7,
    5.08e-7 and 5.00e-7 in the order of the cases, against a ceiling of 2e-4: the assert is four times each figure."""
    ctx = gpu_ctx
    rng = np.random.default_rng(7 * D + K)
    x = rng.standard_normal((D, T)).astype(np.float32)
    basis = _orthonormal(rng, D, K)
    ld = ctx.lib.pmd_time_ld(T) + (64 if K in (3, 65) else 0)
    ldp = ld + 32
    xs = _padded(ctx, x, -(-D // 1024) * 1024, ld)
    bd = _dev(ctx, basis)
    pj = _nan(ctx, K + SENTINELS, ldp)
    ws = _workspace(ctx, ctx.lib.pmd_bg_project_workspace_bytes(D, T))
    ctx.call("pmd_bg_project", P(xs), D, T, ld, P(bd), K, P(pj), ldp, P(ws), ws.numel())
    ctx.sync()
    assert _untouched(pj[K:])
    got = pj[:K, :T].cpu().numpy()
    ref = R.project_ref(basis, x)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"\nbg_project D={D} T={T} K={K}: max err / max|ref| = {err:.3g}")
    assert np.all(np.isfinite(got))
    assert err <= PROJECT_TOL[(D, T, K)]


# ---------------------------------------------------------------------------------------------- pmd_bg_filter
@pytest.mark.parametrize("D,nf,K", [(360, 120, 3), (70, 257, 16), (70, 257, 17), (129, 300, 64), (129, 300, 65), (61, 5, 1)])
def test_bg_filter(gpu_ctx, D, nf, K):
    """X - B pj with a random pj that is not derived from the data, so the filter's own error stays visible.  Elementwise
    |got - ref| <= (K + 4) 2^-24 (|x| + sum_k |b_k| |pj_k|): one fma chain of K terms, one subtraction, one stored rounding
    per extra pass of 64 columns.  Columns [nf, ld) are exact zeros, and the in-place call gives the bits of the
    out-of-place one.  Measured on an MI355X: the largest error is 0.23 of the bound (K = 3), 0.04 to 0.05 of it at K = 64, 65."""
    ctx = gpu_ctx
    rng = np.random.default_rng(11 * D + K)
    x = rng.standard_normal((D, nf)).astype(np.float32)
    basis = _orthonormal(rng, D, K)
    pj_np = rng.standard_normal((K, nf)).astype(np.float32)
    ld = ctx.lib.pmd_time_ld(nf) + (64 if K in (3, 17, 65) else 0)
    ldp = ld + 96
    xs = _padded(ctx, x, D + SENTINELS, ld)
    bd = _dev(ctx, basis)
    pj = _padded(ctx, pj_np, K, ldp)
    out = _nan(ctx, D + SENTINELS, ld)
    ctx.call("pmd_bg_filter", P(xs), P(out), D, nf, ld, P(bd), K, P(pj), ldp)
    ctx.sync()
    assert _untouched(out[D:])
    got = out[:D].cpu().numpy()
    assert np.all(_bits(got[:, nf:]) == 0)
    ref = R.filter_ref(x, basis, pj_np)
    ratio = np.abs(got[:, :nf] - ref) / R.filter_bound(x, basis, pj_np, K)
    print(f"\nbg_filter D={D} nf={nf} K={K}: err / bound = {ratio.max():.3g}")
    assert np.all(ratio <= 1.0)
    # in place: the sentinel rows of the input array are NaN this time, and stay so
    xs[D:] = float("nan")
    ctx.call("pmd_bg_filter", P(xs), P(xs), D, nf, ld, P(bd), K, P(pj), ldp)
    ctx.sync()
    assert _untouched(xs[D:])
    assert np.array_equal(_bits(xs[:D].cpu().numpy()), _bits(got))


# ---------------------------------------------------------------------------------------------- pmd_scale_rows
@pytest.mark.parametrize("D,nf", [(117, 120), (32768 + 70, 3)])
def test_scale_rows(gpu_ctx, D, nf):
    """x[c][f] *= w[c]: the bits of the fp32 product, rows on both sides of the split into launches of 32768 rows, columns
    from nf on and the rows beyond D unchanged."""
    ctx = gpu_ctx
    rng = np.random.default_rng(D)
    x = rng.standard_normal((D, nf)).astype(np.float32)
    w = (0.5 + rng.random(D)).astype(np.float32)
    ld = ctx.lib.pmd_time_ld(nf) + (64 if nf == 120 else 0)
    xd = _padded(ctx, x, D + SENTINELS, ld, fill=7.0)
    xd[D:] = float("nan")
    wd = _dev(ctx, w)
    ctx.call("pmd_scale_rows", P(xd), D, nf, ld, P(wd))
    ctx.sync()
    assert _untouched(xd[D:])
    got = xd[:D].cpu().numpy()
    assert np.all(got[:, nf:] == 7.0)
    assert np.array_equal(_bits(got[:, :nf]), _bits(x * w[:, None]))
    assert np.all(np.abs(got[:, :nf] - R.scale_rows_ref(x, w)) <= EPS * np.abs(R.scale_rows_ref(x, w)))


# ---------------------------------------------------------------------------------------------- pmd_background_rsvd
RSVD_SEED = 77


def _rsvd_input(D, n, K, ratio):
    """K + 6 planted components with singular values 100 ratio^k and orthonormal factors, plus N(0, 0.02^2)."""
    rng = np.random.default_rng(1)
    r = K + 6
    u = np.linalg.qr(rng.standard_normal((D, r)))[0]
    v = np.linalg.qr(rng.standard_normal((n, r)))[0]
    return ((u * (100.0 * ratio ** np.arange(r))) @ v.T + 0.02 * rng.standard_normal((D, n))).astype(np.float32)


def _run_rsvd(ctx, x, K, extra_ld):
    D, n = x.shape
    ld = ctx.lib.pmd_time_ld(n) + extra_ld
    xs = _padded(ctx, x, -(-D // 1024) * 1024, ld)
    basis = _nan(ctx, D + SENTINELS, K)
    ws = _workspace(ctx, ctx.lib.pmd_background_rsvd_workspace_bytes(D, n, K))
    ctx.call("pmd_background_rsvd", P(xs), D, n, ld, K, RSVD_SEED, P(basis), P(ws), ws.numel())
    ctx.sync()
    assert _untouched(basis[D:])
    return basis[:D].cpu().numpy()


def _check_rsvd(got, ref, oracle_basis, K, label):
    e32 = R.column_distance(oracle_basis, ref)
    dist = R.column_distance(got, ref)
    orth = np.abs(got.astype(np.float64).T @ got.astype(np.float64) - np.eye(K)).max()
    sgn = np.where(np.sum(got * ref, axis=0) < 0, -1.0, 1.0)
    overall = np.linalg.norm(got * sgn - ref) / np.linalg.norm(ref)
    print(f"\nrsvd {label}: column distance {dist:.3g}, fp32 oracle's e32 {e32:.3g} (ratio {dist / e32:.3g}), "
          f"orthonormality {orth:.3g}, overall rel {overall:.3g}")
    assert np.all(np.isfinite(got))
    assert orth < 1e-5
    assert dist <= max(8 * e32, 1e-6)
    assert overall < 2e-4


@pytest.mark.parametrize("D,n,K,ratio", [(100, 80, 4, 0.7), (257, 90, 3, 0.7), (300, 100, 1, 0.7), (1500, 200, 16, 0.8),
                                         (700, 130, 54, 0.9), (700, 130, 55, 0.9)])
def test_background_rsvd(gpu_ctx, D, n, K, ratio):
    """The basis against the float64 rSVD of the same input with the device's own Omega: orthonormal to 1e-5; after sign
    alignment the largest per-column L2 distance is at most max(8 e32, 1e-6), e32 being the same distance for the oracle's
    fp32 rSVD (oracle.loader_truncated_random_svd) on the same input, computed here: the factor 8 covers the kernel's other
    summation order and its Gram-route SVD at equal operand precision.  The suite's overall rel_err < 2e-4 stays as a
    ceiling.  K = 54 is the full width (64 sketch columns) of the Cholesky path, K = 55 the first on the generic-width
    kernels; D = 257, 300, 700 and 1500 leave a ragged last block of 256 pixels.
    Measured on an MI355X, column distance / e32 in the order of the cases: 1.9e-7 / 2.9e-7, 1.8e-7 / 2.9e-7, 8.0e-8 / 1.5e-7,
    1.5e-6 / 2.7e-6, 2.3e-5 / 3.2e-5, 3.0e-5 / 9.2e-5: the kernel is closer to float64 than the fp32 oracle in every case;
    overall rel_err at most 8.5e-6."""
    ctx = gpu_ctx
    x = _rsvd_input(D, n, K, ratio)
    got = _run_rsvd(ctx, x, K, 64 if K in (3, 55) else 0)
    omega = DeviceSource(ctx, RSVD_SEED).omega(philox.STREAM_BG_OMEGA, 0, n, K + 10)
    ref = R.rsvd_ref(x, omega, K)[0]
    oracle_basis, _ = O.loader_truncated_random_svd(x, omega, K)
    _check_rsvd(got, ref, oracle_basis, K, f"D={D} n={n} K={K}")


def test_background_rsvd_fewer_frames_than_sketch_columns(gpu_ctx):
    """12 sample frames, 14 sketch columns: the sketch spans the whole row space, the rSVD is exact, and the expected basis
    is the top four left singular vectors of the input in float64.  Measured on an MI355X: column distance 5.8e-7, e32 8.2e-7."""
    ctx = gpu_ctx
    D, n, K = 300, 12, 4
    x = _rsvd_input(D, n, K, 0.7)
    got = _run_rsvd(ctx, x, K, 0)
    omega = DeviceSource(ctx, RSVD_SEED).omega(philox.STREAM_BG_OMEGA, 0, n, K + 10)
    ref = np.linalg.svd(x.astype(np.float64), full_matrices=False)[0][:, :K]
    oracle_basis, _ = O.loader_truncated_random_svd(x, omega, K)
    _check_rsvd(got, ref, oracle_basis, K, f"D={D} n={n} K={K} (degenerate)")


# ---------------------------------------------------------------------------------------------- pmd_threshold_sim
SIM_SEED = 5


@pytest.mark.parametrize("b1,b2,t,iters", [(10, 12, 64, 8), (10, 12, 65, 8), (20, 20, 500, 12), (16, 10, 40, 300)])
def test_threshold_sim(gpu_ctx, b1, b2, t, iters):
    """Both roughness statistics of every iteration against the float64 rank-1 rSVD of the device's own noise tile and
    sketch, rtol 2e-4 (the suite's present tolerance, now against float64; the fp32 oracle itself is within 4.1e-6 of
    float64 on these draws, and the first two singular values are never closer than 1.6e-3 relative).  300 iterations span
    two batches of 256: iteration 256 must draw array 256 and land in row 256.  The tiles are not square, so a b1 / b2 swap
    in the spatial statistic shows.
    Measured on an MI355X, largest relative distance (spatial, temporal): 1.8e-7, 2.6e-7; 1.9e-7, 1.4e-7; 1.9e-7, 2.5e-7;
    9.0e-7, 3.6e-6 over the 300 iterations."""
    ctx = gpu_ctx
    ws = _workspace(ctx, ctx.lib.pmd_threshold_sim_workspace_bytes(b1, b2, t, iters))
    out = _nan(ctx, iters + SENTINELS, 2)
    ctx.call("pmd_threshold_sim", b1, b2, t, iters, SIM_SEED, P(out), P(ws), ws.numel())
    ctx.sync()
    assert _untouched(out[iters:])
    got = out[:iters].cpu().numpy().astype(np.float64)
    src = DeviceSource(ctx, SIM_SEED)
    ref = np.array([R.sim_ref(src.noise(k, b1, b2, t), src.omega(philox.STREAM_SIM_OMEGA, k, t, 11)) for k in range(iters)])
    rel = np.abs(got - ref) / np.abs(ref)
    print(f"\nthreshold_sim {b1}x{b2}x{t}, {iters} iterations: rel spatial {rel[:, 0].max():.3g} temporal {rel[:, 1].max():.3g}")
    np.testing.assert_allclose(got[:, 0], ref[:, 0], rtol=2e-4, atol=0)
    np.testing.assert_allclose(got[:, 1], ref[:, 1], rtol=2e-4, atol=0)
