"""
The first temporal window of the tile stage on constant, dead and low-rank tiles (GPU): pmd_tiles_decompose /
pmd_tiles_decompose_staged called by name through the C ABI on the family of tests/tile_stage_ref.py (KINDS: an all-zero
tile, tiles of rank 3, 1 and 2 made of small integers, a planted tile with dead image rows and a dead column, two ordinary
planted tiles), all kinds in ONE launch of disjoint tiles.  tests/test_tile_stage_ref.py proves on the CPU that the family is
admissible.  Before every call the workspace and every output hold 0xFF bytes and a guard tile stands behind each output
(tile_stage_ref.device_run).

Three forms: Zn (r = 6, pooling 2: 64 rows, Cholesky whitening), Zw (r = 60, no pooling, 400 frames: 128 rows, the
generic-width path) and Zn through the staged entry point (stages 1, 2, 4: the eigenvector whitening).

What is promised ("All-constant tiles"): ranks as in the reference, zero vectors for the null directions of
an all-zero tile, the same reconstruction.
"""
import numpy as np
import pytest

from tests import test_gpu_tile_stage as S
from tests import tile_stage_ref as R
from tests.util import DeviceSource

pytestmark = pytest.mark.gpu

FORMS = {"Zn": ("Zn", False), "Zw": ("Zw", False), "Zn-staged": ("Zn", True)}

# device <= FACTOR x fp32 oracle (single-precision LAPACK) for the three measures of a degenerate tile.  The rule of
# test_gpu_tile_stage.py: the smallest power of two at or above twice the largest ratio measured on MI355X, never below 4.
# Largest ratios: residual 0.85 (Zw low3), singular values 0.27 (rank1), orthonormality 1.33 (Zn rank1: 2.98e-8 against
# 2.24e-8, both at the rounding of one fp32 entry), so every factor is the floor, 4.  The figures are in the docstring of
# test_degenerate_tiles.
FACTOR = {"rec": 4.0, "sigma": 4.0, "orth": 4.0}

_ORACLES = {}
_RUNS = {}


def _oracles(ctx, name):
    """The float64 oracle and the fp32 oracle with single-precision LAPACK of every tile on the device's omegas, computed
    once per case and left unchanged."""
    if name not in _ORACLES:
        _ORACLES[name] = R.case_oracles(name, DeviceSource(ctx, R.SEED), modes=("f64", "f32s"))
    return _ORACLES[name]


def _run(ctx, form, max_fail):
    """The launch of all tiles under the case's own thresholds, once per (form, max_fail)."""
    if (form, max_fail) not in _RUNS:
        name, staged = FORMS[form]
        _RUNS[(form, max_fail)] = R.device_run(ctx, name, R.thresholds(name)[0], max_fail, staged=staged)
    return _RUNS[(form, max_fail)]


def _tile_matrix(name, t):
    d = R.tile_block(name, t).shape[0] * R.tile_block(name, t).shape[1]
    return R.movie_rows(name)[t * d:(t + 1) * d].astype(np.float64)


def _measures(X, u, v, sig, rho):
    """(relative residual of u v over all components, largest relative error of the rho leading singular values against
    float64, orthonormality defect of the rho leading columns of u)."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    sv = np.linalg.svd(X, compute_uv=False)[:rho]
    rec = float(np.linalg.norm(X - u @ v) / np.linalg.norm(X))
    sigma = float(np.max(np.abs(np.asarray(sig, dtype=np.float64)[:rho] - sv) / sv))
    orth = float(np.abs(u[:, :rho].T @ u[:, :rho] - np.eye(rho)).max())
    return {"rec": rec, "sigma": sigma, "orth": orth}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


@pytest.mark.parametrize("form", list(FORMS))
def test_degenerate_tiles(gpu_ctx, form):
    """Every kind in one launch, the case's own thresholds, max_fail in {1, 2, 3}.

    Every run: Ut, V and lam finite everywhere, all three exactly zero for the all-zero tile; rows from r_eff on and the
    padding zero, guard tiles unchanged (device_run); good, keep and ranks follow exactly from the returned statistics, a
    NaN statistic (0 / 0 of a zero vector) counting as a failure.  Every row c of Ut has norm <= 1 + 1e-5 and its V row
    has norm sqrt(lam_c) within r_eff 2^-24 sqrt(lam_0) (a V row is an fp32 mix of r_eff rows no longer than sqrt(lam_0)).
    The degenerate kinds: exactly rho components with sqrt(lam) > 1e-3 sqrt(lam_0); good is 1 on them and 0 elsewhere;
    ranks = rho + min(max_fail, r_eff - rho), which at max_fail = 1 is the float64 oracle's rank (not compared beyond:
    the oracle's null vectors are LAPACK's arbitrary ones and pass by chance).

    Accuracy of the tiles of rank 3, 1 and 2, device <= FACTOR x fp32 oracle with single-precision LAPACK on the same
    inputs: || X - Ut^T V ||_F / || X ||_F over all rows, the relative error of sqrt(lam[:rho]) against the float64
    singular values, the orthonormality defect of the rho strong rows of Ut.  The deadrows tile and the two live tiles go
    through the comparison of test_gpu_tile_stage.py (K_device <= FACTOR x K_oracle32 for U, V, sqrt(lam) and the two
    statistics, subspace, orthonormality, decisions against the float64 oracle).

    Measured on MI355X, device / fp32 oracle in the order residual, sqrt(lam), orthonormality:
      Zn        low3 1.28e-7 / 3.26e-7, 1.83e-8 / 2.35e-7, 1.79e-8 / 2.14e-7; rank1 3.34e-7 / 7.38e-7, 4.16e-8 / 1.56e-7,
                2.98e-8 / 2.24e-8; sparse2 8.87e-9 / 4.93e-8, 1.02e-9 / 1.16e-8, 0 / 0
      Zw        low3 4.17e-7 / 4.92e-7, 1.58e-8 / 9.84e-8, 3.32e-8 / 3.68e-8; rank1 3.25e-7 / 1.26e-6, 2.63e-8 / 1.09e-7,
                2.98e-8 / 2.01e-7; sparse2 9.32e-9 / 3.98e-7, 1.13e-10 / 2.02e-8, 0 / 1.19e-7
      Zn-staged low3 1.42e-7 / 3.26e-7, 1.14e-8 / 2.35e-7, 1.58e-8 / 2.14e-7; rank1 3.34e-7 / 7.38e-7, 4.16e-8 / 1.56e-7,
                2.98e-8 / 2.24e-8; sparse2 8.07e-9 / 4.93e-8, 2.38e-10 / 1.16e-8, 0 / 0
    (the two live pixels of sparse2 give unit vectors: the defect is exactly zero on both sides, and 0 <= 4 x 0 holds).
    The deadrows and live tiles, largest ratio device / fp32 oracle over U, V, sqrt(lam) and the two statistics: Zn 0.47,
    Zw 0.53, Zn-staged 0.56 (each the temporal statistic or sqrt(lam)); 6 separated components per tile in Zn, 48, 44 and
    45 in Zw; no (tile, threshold pair) under the knife-edge exemption."""
    ctx = gpu_ctx
    name, staged = FORMS[form]
    own = R.thresholds(name)[0]
    refs = _oracles(ctx, name)
    re = R.r_eff(name)
    problems = []
    runs = {}
    for mf in R.MAX_FAILS:
        run = runs[mf] = _run(ctx, form, mf)
        torch = S._t()
        assert bool(torch.isfinite(run.dev_ut[:run.n]).all()), "Ut"
        assert bool(torch.isfinite(run.dev_v[:run.n, :, :run.T]).all()), "V"
        assert np.all(np.isfinite(run.lam)), "lam"
        R.check_decisions(name, run, own, mf, set())
        for t, kind in enumerate(R.KINDS):
            lam = run.lam[t, :re]
            s = np.sqrt(np.maximum(lam, 0.0))
            un = np.linalg.norm(run.ut[t].astype(np.float64), axis=1)
            vn = np.linalg.norm(run.v[t].astype(np.float64), axis=1)
            if np.any(un > 1 + 1e-5):
                problems.append((mf, kind, "norm of a Ut row", float(un.max())))
            if np.any(np.abs(vn - s) > re * 2.0 ** -24 * s[0]):
                problems.append((mf, kind, "V row norm against sqrt(lam)", float(np.abs(vn - s).max()), float(s[0])))
            if kind not in R.RHO:
                continue
            rho = R.RHO[kind]
            if kind == "zero":
                if run.ut[t].any() or run.v[t].any() or run.lam[t].any():
                    problems.append((mf, kind, "the all-zero tile is not exactly zero"))
            strong = int(np.sum(s > 1e-3 * s[0])) if rho else int(np.sum(s > 0))
            if strong != rho:
                problems.append((mf, kind, "strong components", strong, s[:rho + 2].tolist()))
            expected_good = (np.arange(re) < rho).astype(np.int32)
            if not np.array_equal(run.good[t, :re], expected_good):
                problems.append((mf, kind, "good", run.good[t, :re].tolist(), run.stats[t, :min(re, rho + 3)].tolist()))
            if run.ranks[t] != rho + min(mf, re - rho):
                problems.append((mf, kind, "rank", int(run.ranks[t]), rho + min(mf, re - rho)))
            if mf == 1 and run.ranks[t] != R.oracle_rank(refs[t]["f64"], own, 1):
                problems.append((mf, kind, "rank against the float64 oracle", int(run.ranks[t])))
    run = runs[1]
    for t, kind in enumerate(R.KINDS):
        if not R.RHO.get(kind):
            continue
        rho, X, r32 = R.RHO[kind], _tile_matrix(name, t), refs[t]["f32s"]
        dev = _measures(X, run.ut[t].T, run.v[t], np.sqrt(np.maximum(run.lam[t, :re], 0.0)), rho)
        ref = _measures(X, r32.u, r32.v, np.linalg.norm(r32.v.astype(np.float64), axis=1), rho)
        print(f"\n{form} {kind}: " + ", ".join(f"{m} device {dev[m]:.2e} / fp32 oracle {ref[m]:.2e} (x{dev[m] / ref[m] if ref[m] else np.inf:.2f})"
                                                for m in dev))
        for m in dev:
            if not dev[m] <= FACTOR[m] * ref[m]:
                problems.append((kind, m, dev[m], ref[m]))
    assert not problems, problems
    ids = [t for t, kind in enumerate(R.KINDS) if kind not in R.RHO]
    K, seps, knife = S._compare(name, runs[3], {own: runs[1]}, refs, ids)
    assert min(s[0] for s in seps) >= 3
    S._report_and_assert(name, form, K, seps, knife, len(ids))


@pytest.mark.parametrize("form", list(FORMS))
def test_live_tiles_do_not_see_their_degenerate_neighbours(gpu_ctx, form):
    """The bits of every output of the two live tiles in the launch of all kinds equal their bits in a launch that holds
    only those two tiles (same sketch matrices; both launches have fewer than 4096 tiles and share a slice plan)."""
    ctx = gpu_ctx
    name, staged = FORMS[form]
    mixed = _run(ctx, form, 1)
    first = R.LIVE_TILES[0]
    assert R.LIVE_TILES == (first, first + 1) and all(R.KINDS[t] == "live" for t in R.LIVE_TILES)
    alone = R.device_run(ctx, name, R.thresholds(name)[0], 1, n_tiles=2, staged=staged, first_tile=first)
    for what in ("ut", "v", "stats", "lam", "good", "keep", "ranks"):
        a, b = getattr(alone, what), getattr(mixed, what)[first:first + 2]
        assert np.array_equal(_bits(a), _bits(b)), (form, what, int(np.sum(_bits(a) != _bits(b))))


@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("form", list(FORMS))
def test_scale_covariance(gpu_ctx, form, scale):
    """The whole family multiplied by 2^24 and by 2^-24: Ut, both statistics, good, keep and ranks are bit-identical, V is
    the exact power-of-two multiple and lam is scaled by 2^48 / 2^-48: every tolerance in the path is relative.  This
    holds on all three forms, the rocSOLVER step of the wide path included.  It did not before small_qr_kernel took its
    relative dependence rule: the Householder QR of the sketch of the rank1 tile (identical rows) reflected on rounding
    residue of rounding residue until the squares underflowed, the null columns of Q then depended on the scale, and at
    2^-24 the leading pair of Ut and V came out with the other sign."""
    ctx = gpu_ctx
    name, staged = FORMS[form]
    base = _run(ctx, form, 1)
    scaled = R.device_run(ctx, name, R.thresholds(name)[0], 1, staged=staged, scale=scale)
    problems = []
    for t, kind in enumerate(R.KINDS):
        checks = {
            "Ut": np.array_equal(_bits(scaled.ut[t]), _bits(base.ut[t])),
            "stats": np.array_equal(scaled.stats[t], base.stats[t], equal_nan=True),
            "good": np.array_equal(scaled.good[t], base.good[t]),
            "keep": np.array_equal(scaled.keep[t], base.keep[t]),
            "ranks": scaled.ranks[t] == base.ranks[t],
            "V": np.array_equal(scaled.v[t], base.v[t] * np.float32(scale)),
            "lam": np.array_equal(scaled.lam[t], base.lam[t] * (scale * scale)),
        }
        for what, ok in checks.items():
            if not ok:
                detail = ""
                if what == "Ut":
                    rows = np.nonzero((_bits(scaled.ut[t]) != _bits(base.ut[t])).any(axis=1))[0]
                    detail = f"rows {rows.tolist()[:8]} max diff {float(np.abs(scaled.ut[t] - base.ut[t]).max()):.2e}"
                if what == "V":
                    rows = np.nonzero((scaled.v[t] != base.v[t] * np.float32(scale)).any(axis=1))[0]
                    detail = f"rows {rows.tolist()[:8]}"
                if what == "lam":
                    rows = np.nonzero(scaled.lam[t] != base.lam[t] * (scale * scale))[0]
                    detail = f"entries {rows.tolist()[:8]} {(scaled.lam[t][rows[:4]] / (scale * scale)).tolist()} {base.lam[t][rows[:4]].tolist()}"
                problems.append((t, kind, what, detail))
    assert not problems, problems
