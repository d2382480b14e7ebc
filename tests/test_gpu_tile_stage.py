"""
The first temporal window of the tile stage (GPU): pmd_tiles_decompose / pmd_tiles_decompose_staged called by name through
the C ABI, at every width, against the float64 oracle of the same operation (oracle.pmd_oracle.single_block_md under
arbiter_precision) fed with the device's own sketch matrices.

The inputs are planted movies over a small field of view (tests/tile_stage_ref.py; tests/test_tile_stage_ref.py proves on
the CPU that they are admissible), the tiles lie on the driver's overlapping grid.  Before every call the workspace and
every output hold NaN bytes, and a guard tile stands behind each output.

Accuracy is measured in units of the reference's own fp32 error: with K = max over the separated components of
rel_err_c gap_c sig_c / s0 (the constant of the bound K s0 / (gap_c sig_c), s0 the largest singular value of the tile
block), the assertion is K_device <= FACTOR x K_oracle32 (FACTOR below), where K_oracle32 is the same quantity of the fp32 oracle with
single-precision LAPACK against the float64 oracle, evaluated in the test on the same inputs; likewise for the relative
errors of sqrt(lam) and of the two statistics.
"""
import numpy as np
import pytest

from tests import tile_stage_ref as R
from tests.util import DeviceSource, context_under, rel_err

pytestmark = pytest.mark.gpu

# K_device <= FACTOR x K_oracle32.  The rule: the smallest power of two at or above twice the largest ratio measured on MI355X
# (twice: another summation order on other inputs), never below 4.  Applied to the vector measures (U, V and the hook arrays:
# largest ratio 1.09, V_ds of the staged case) and to the scalar ones (sqrt(lam) and the two statistics: largest ratio 2.27,
# the temporal statistic of case F2q) separately; one factor for all would be 8.  The figures are in the docstring of
# test_tiles_decompose_vs_float64_oracle.
FACTOR = {"U": 4.0, "V": 4.0, "V_ds": 4.0, "S": 4.0, "sigma": 8.0, "spatial": 8.0, "temporal": 8.0}
METRICS = ("U", "V", "sigma", "spatial", "temporal")


def _t():
    import torch

    return torch


# the call itself, its guard tiles and the exact check of the decisions are shared with tests/test_gpu_tile_degenerate.py
_device_run = R.device_run
_check_decisions = R.check_decisions


_ORACLES = {}


def _oracles(ctx, name, tile_ids=None):
    """The float64 oracle and the fp32 oracle with single-precision LAPACK of the tiles of a case on the device's omegas,
    computed once per case and left unchanged."""
    if name not in _ORACLES:
        _ORACLES[name] = R.case_oracles(name, DeviceSource(ctx, R.SEED), tile_ids, modes=("f64", "f32s"))
    return _ORACLES[name]


def _compare(name, run, runs_mf1, refs, tile_ids, hooks=None):
    """The pass-everything run against the float64 oracle, tile by tile.  Returns ({metric: (K_device, K_oracle32)},
    separated components per tile, (tile, threshold pair) under the knife-edge exemption)."""
    re, d = run.re, run.d
    K = {m: [0.0, 0.0] for m in METRICS + (("V_ds", "S") if hooks is not None else ())}
    seps, knife = [], 0

    def note(metric, dev, ref32):
        K[metric][0] = max(K[metric][0], dev)
        K[metric][1] = max(K[metric][1], ref32)

    for t in tile_ids:
        r64, r32 = refs[t]["f64"], refs[t]["f32s"]
        assert r64.u.shape == (d, re)
        sig = np.linalg.norm(r64.v, axis=1)
        gaps, strong, sep = R.separation(sig)
        seps.append((int(sep.sum()), int(sep[64:].sum()), int(sep[128:].sum())))
        s0 = R.block_s0(name, t)
        u_got = run.ut[t].T.astype(np.float64)
        v_got = run.v[t].astype(np.float64)
        note("sigma", R.scalar_K(np.sqrt(np.maximum(run.lam[t, :re], 0)), sig, sep), R.scalar_K(np.linalg.norm(r32.v, axis=1), sig, sep))
        note("U", R.vector_K(u_got, r64.u, sig, s0, sep, 0), R.vector_K(r32.u, r64.u, sig, s0, sep, 0))
        note("V", R.vector_K(v_got, r64.v, sig, s0, sep, 1), R.vector_K(r32.v, r64.v, sig, s0, sep, 1))
        note("spatial", R.scalar_K(run.stats[t, :re, 0], r64.sp, sep), R.scalar_K(r32.sp, r64.sp, sep))
        note("temporal", R.scalar_K(run.stats[t, :re, 1], r64.tp, sep), R.scalar_K(r32.tp, r64.tp, sep))
        if hooks is not None:
            sep_ds = R.separation(r64.s_ds)[2]
            note("V_ds", R.vector_K(hooks.v_ds[t], r64.v_ds, r64.s_ds, r64.s_ds[0], sep_ds, 1),
                 R.vector_K(r32.v_ds, r64.v_ds, r64.s_ds, r64.s_ds[0], sep_ds, 1))
            sig_b = np.linalg.svd(r64.v_ds, compute_uv=False)
            sep_b = R.separation(sig_b)[2]
            assert sep_ds.sum() >= 30 and sep_b.sum() >= 30, (name, t, int(sep_ds.sum()), int(sep_b.sum()))
            note("S", R.vector_K(hooks.S[t].T, r64.S, sig_b, sig_b[0], sep_b, 0), R.vector_K(r32.S, r64.S, sig_b, sig_b[0], sep_b, 0))
        ns = int(strong.sum())
        assert np.all(strong[:ns])
        proj = r64.u[:, :ns] @ (r64.u[:, :ns].T @ u_got[:, :ns])
        sub = rel_err(proj, u_got[:, :ns])
        assert sub < 5e-3, (name, t, ns, sub)
        orth = float(np.abs(u_got[:, :ns].T @ u_got[:, :ns] - np.eye(ns)).max())
        assert orth < 2e-5, (name, t, orth)
        for thr, run1 in runs_mf1.items():
            dev_stats = run1.stats[t, :re][strong]
            if R.margin_ok(r64.sp[strong], r64.tp[strong], thr) and R.margin_ok(dev_stats[:, 0], dev_stats[:, 1], thr):
                good_ref = (r64.sp < thr[0]) & (r64.tp < thr[1])
                np.testing.assert_array_equal(run1.good[t, :re][strong] > 0, good_ref[strong], err_msg=f"{name} tile {t} {thr}")
            else:
                knife += 1
    return K, seps, knife


def _report_and_assert(name, label, K, seps, knife, n_pairs):
    ratios = {m: (K[m][0] / K[m][1] if K[m][1] > 0 else float("inf")) for m in K}
    print(f"\ncase {name} {label}: " + ", ".join(f"{m} device {K[m][0]:.2e} / fp32 oracle {K[m][1]:.2e} (x{ratios[m]:.2f})" for m in K)
          + f"; separated per tile (all, >= 64, >= 128) {seps[:6]}{' ...' if len(seps) > 6 else ''}; knife-edge share {knife / n_pairs:.2f}")
    if name in R.MIN_SEPARATED:
        need = R.MIN_SEPARATED[name]
        assert all(s[0] >= need[0] and s[1] >= need[1] and s[2] >= need[2] for s in seps), (name, seps)
    assert knife / n_pairs <= 0.10, (name, knife)
    for m in K:
        assert K[m][1] > 0 and K[m][0] <= FACTOR[m] * K[m][1], (name, label, m, K[m], ratios[m], FACTOR[m])


def _case(ctx, name, label, staged=False):
    thresholds = R.thresholds(name)
    patterns, runs = set(), {}
    for thr in thresholds:
        for mf in R.MAX_FAILS:
            run = _device_run(ctx, name, thr, mf, staged=staged)
            _check_decisions(name, run, thr, mf, patterns)
            runs[(thr, mf)] = run
    assert patterns == {"pass after a failure", "cut by max_fail"}, (name, patterns)
    refs = _oracles(ctx, name)
    run = runs[(R.PASS_ALL, 3)]
    assert np.all(run.ranks == run.re), "the pass-everything run keeps every component"
    K, seps, knife = _compare(name, run, {thr: runs[(thr, 1)] for thr in thresholds}, refs, range(run.n), hooks=run if staged else None)
    _report_and_assert(name, label, K, seps, knife, run.n * len(thresholds))


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "F1w", "F1n", "F2p", "F2q"])
def test_tiles_decompose_vs_float64_oracle(gpu_ctx, name):
    """pmd_tiles_decompose on the planted cases of tile_stage_ref.CASES: A (r = 54: l = 64 = rp, the last 64-row width,
    Householder QR in LDS), B (r = 55: l = 65, rp = 128, the first generic width), C (r = 80: components in two row
    blocks, 90 sketch rows < 100 pooled pixels), D (r = 150: rp = 192, three row blocks), E (30 x 30 tiles without
    pooling: the sketch does not fit LDS, CholeskyQR2 basis on the 64-row path), F1w / F1n (r = 80 / 20 clamped to 10 time
    bins, at both widths), F2p / F2q (10 x 10 tiles, r = 95 clamped to 25 pooled pixels / d = 100 < l).  Both threshold
    pairs with max_fail in {1, 2, 3}.

    Every run: good, keep and ranks follow exactly from the statistics the device returned (filter_by_failures); rows from
    r_eff = min(r, bins, pooled pixels) on of Ut, V, stats, good, keep and lam_out are zero; the guard tiles are unchanged;
    over the runs of a case a pass after a failure and a cut by max_fail both occur.

    The pass-everything run against the float64 oracle per tile: K_device <= FACTOR x K_oracle32 for the U columns and V
    rows of the separated components (gap > 2e-2, sig > 1e-3 sig_0) after sign alignment, for sqrt(lam) against the trace
    norms and for the two statistics; subspace of the strong components within 5e-3; orthonormality below 2e-5; good equal
    to the oracle's wherever both sides are farther than KNIFE_EDGE from the threshold (at most 10 % of (tile, threshold
    pair) exempt).  At least 30 separated components per tile in A-E, 5 beyond row 64 in C and D, 5 beyond row 128 in D.

    Measured on MI355X, device / fp32 oracle (the bound is FACTOR times the second figure: 4 for U and V, 8 for the three
    scalar measures), in the order U, V, sqrt(lam), spatial statistic, temporal statistic:
      A   3.30e-8 / 3.27e-7, 1.25e-7 / 3.78e-7, 5.12e-7 / 2.16e-6, 4.98e-7 / 5.56e-6, 7.74e-7 / 4.12e-6
      B   8.56e-8 / 3.44e-7, 1.08e-7 / 3.58e-7, 3.00e-7 / 9.34e-7, 5.52e-7 / 4.26e-6, 7.16e-7 / 3.51e-6
      C   1.01e-7 / 5.58e-7, 1.37e-7 / 5.43e-7, 1.55e-6 / 4.26e-6, 1.81e-6 / 4.48e-6, 2.14e-6 / 5.52e-6
      D   8.70e-8 / 3.57e-7, 9.64e-8 / 3.36e-7, 4.02e-6 / 3.77e-6, 4.44e-6 / 8.04e-6, 1.07e-5 / 6.18e-6
      E   3.28e-8 / 3.18e-7, 6.28e-8 / 2.97e-7, 1.09e-7 / 2.04e-6, 3.21e-7 / 6.00e-6, 3.20e-7 / 6.04e-6
      F1w 6.01e-8 / 2.20e-7, 8.87e-8 / 3.43e-7, 1.23e-7 / 1.12e-6, 7.63e-7 / 3.38e-6, 1.45e-6 / 4.29e-6
      F1n 2.76e-8 / 2.00e-7, 8.63e-8 / 2.95e-7, 1.27e-7 / 6.09e-7, 7.03e-7 / 3.47e-6, 2.15e-6 / 9.18e-6
      F2p 1.10e-7 / 2.73e-7, 5.00e-8 / 3.18e-7, 7.58e-8 / 1.81e-6, 3.26e-7 / 5.37e-6, 2.39e-7 / 1.30e-6
      F2q 1.20e-7 / 2.09e-7, 1.29e-7 / 2.74e-7, 3.39e-5 / 2.00e-5, 8.46e-6 / 7.04e-6, 1.33e-5 / 5.86e-6
    Largest ratio device / fp32 oracle: 0.57 for U and V (F2q), 2.27 for the scalar measures (temporal statistic of F2q; 1.73
    in D): the device forms every Gram matrix behind an SVD in fp64 and is ahead of sgesdd on the vectors; where it is
    behind, on the statistics and singular values of tiles with 95 and 150 components, both sides are at a few 1e-5
    relative.  Separated components per tile: A 43, 45, 42, 46; B 44, 46, 43, 44; C 52, 53, 57, 72 (12, 13, 16, 16 from
    row 64 on); D 72, 59, 59, 75 (43, 31, 39, 38 from row 64 on, 13, 10, 11, 16 from row 128 on); E 42, 40, 40, 36; F1 10,
    10, 10, 8; F2p 23, 23, 19, 17; F2q 76, 77, 73, 75.  No (tile, threshold pair) under the knife-edge exemption."""
    _case(gpu_ctx, name, "default routes")


@pytest.mark.parametrize("name,env", [("A", {"PMD_TILE_WHITEN": "eig"}), ("C", {"PMD_WIDE_EIG": "syevd"})])
def test_tiles_decompose_routes(name, env):
    """Case A with the eigenvector form of the two whitening steps and case C with rocSOLVER's divide-and-conquer solver
    at the generic width, each on a context created under its switch: every assertion of the default routes.  Measured on
    MI355X, device / fp32 oracle in the order U, V, sqrt(lam), spatial, temporal: A 3.40e-8 / 3.27e-7, 1.22e-7 / 3.78e-7,
    4.77e-7 / 2.16e-6, 5.81e-7 / 5.56e-6, 6.90e-7 / 4.12e-6; C 1.02e-7 / 5.58e-7, 1.37e-7 / 5.43e-7, 1.34e-6 / 4.26e-6,
    2.31e-6 / 4.48e-6, 2.66e-6 / 5.52e-6."""
    ctx = context_under(env)
    try:
        _case(ctx, name, " ".join(f"{k}={v}" for k, v in env.items()))
    finally:
        ctx.close()


def test_tiles_decompose_staged_hook_arrays(gpu_ctx):
    """Case A through pmd_tiles_decompose_staged in three calls (stages 1, 2, 4), the workspace untouched between them, the
    hook arrays located with pmd_tiles_hook_offsets: every assertion of the one-call form on the final outputs (this form
    takes the eigenvector whitening), and the hook arrays themselves under the same measure: the rows of V_ds at
    *vds_offset against the oracle's v_ds where the singular values of the pooled, binned block are separated, the columns
    of S at *s_offset against block_2d v_mat_basis^T where the singular values of v_ds are separated.  Measured on MI355X,
    device / fp32 oracle: V_ds 1.59e-7 / 1.46e-7, S 7.07e-8 / 3.19e-7; U 3.34e-8 / 3.27e-7, V 1.34e-7 / 3.78e-7, sqrt(lam)
    4.64e-7 / 2.16e-6, spatial 5.81e-7 / 5.56e-6, temporal 7.74e-7 / 4.12e-6."""
    _case(gpu_ctx, "A", "staged", staged=True)


def test_tiles_decompose_many_tiles_across_the_one_slice_switch(gpu_ctx):
    """4225 overlapping 8 x 8 tiles of a 72 x 72 field of view (an origin at every pixel offset), T = 96, r = 6: the entry
    point with the first 4095 tiles (four time slices, partial Gram matrices, reduce_slices) and with the first 4096 (one
    slice).  Both calls: decisions exact from the returned statistics and orthonormality below 2e-5 on all tiles, zeros
    from r_eff on, guard tiles; the sampled tiles of tile_stage_ref.many_sample (64, with tiles 0, 4094 and 4095, each
    with at least 3 separated components) against the float64 oracle under the measure of the other cases.  Measured on
    MI355X, device / fp32 oracle in the order U, V, sqrt(lam), spatial, temporal: 4095 tiles 5.16e-8 / 2.37e-7,
    4.58e-8 / 3.85e-7, 2.62e-7 / 3.74e-6, 3.47e-7 / 7.51e-6, 3.98e-6 / 1.73e-5; 4096 tiles 1.08e-7 / 2.37e-7,
    4.40e-8 / 3.85e-7, 2.98e-7 / 3.74e-6, 7.89e-7 / 7.51e-6, 2.23e-6 / 1.73e-5."""
    ctx, torch = gpu_ctx, _t()
    name = "many"
    thresholds = R.thresholds(name)
    sample = R.many_sample()
    refs = _oracles(ctx, name, sample)
    for t in sample:
        assert R.separation(np.linalg.norm(refs[t]["f64"].v, axis=1))[2].sum() >= 3, t
    for n in R.MANY_CALLS:
        patterns, runs = set(), {}
        for thr in thresholds:
            for mf in R.MAX_FAILS:
                full = thr == R.PASS_ALL and mf == 3
                run = _device_run(ctx, name, thr, mf, n_tiles=n, download=False)
                _check_decisions(name, run, thr, mf, patterns)
                if full:
                    u = run.dev_ut[:n, :run.re, :run.d].double()
                    gram = torch.bmm(u, u.transpose(1, 2)) - torch.eye(run.re, dtype=torch.float64, device=ctx.device)
                    orth = float(gram.abs().max())
                    assert orth < 2e-5, (n, orth)
                    ids = torch.as_tensor([t for t in sample if t < n], device=ctx.device)
                    run.ids = [t for t in sample if t < n]
                    run.ut = {t: x for t, x in zip(run.ids, run.dev_ut[ids][:, :run.re, :run.d].cpu().numpy())}
                    run.v = {t: x for t, x in zip(run.ids, run.dev_v[ids][:, :run.re, :run.T].cpu().numpy())}
                run.dev_ut = run.dev_v = None
                runs[(thr, mf)] = run
        assert patterns == {"pass after a failure", "cut by max_fail"}, (n, patterns)
        run = runs[(R.PASS_ALL, 3)]
        assert len(run.ids) == (len(sample) if n == 4096 else len(sample) - 1) and {0, 4094} <= set(run.ids)
        K, seps, knife = _compare(name, run, {thr: runs[(thr, 1)] for thr in thresholds}, refs, run.ids)
        assert min(s[0] for s in seps) >= 3
        _report_and_assert(name, f"n = {n}", K, seps, knife, len(run.ids) * len(thresholds))
