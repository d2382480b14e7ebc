"""
The inputs of tests/test_gpu_tile_kernels_wide.py, tests/test_gpu_tile_stage.py and tests/test_gpu_tile_degenerate.py are admissible: proven here on the CPU
from the oracles alone (omegas of oracle.philox.PhiloxSource, which test_rng_matches_numpy_restatement pins to the
device's), before a GPU sees them.
"""
import functools

import numpy as np
import pytest

from oracle import philox
from tests import tile_stage_ref as R

MIN_CLEARANCE = 5 * R.KNIFE_EDGE


@pytest.mark.parametrize("n", R.CHOL_ORDERS)
def test_cholesky_inputs_classify_far_from_the_tolerance(n):
    """Under tol = 1e-10 no pivot of the chosen matrices is a knife edge: every live pivot of the restated rule is above
    1e-4 dmax, every dead one below 1e-12 dmax, the dead rows are the planted ones, the full-rank tiles have
    cond(M) <= 1e4, and the restatement agrees there with inv(cholesky(M)^T)."""
    mats, dead = R.chol_inputs(n)
    G = R.antisymmetric_split(mats, 64, np.random.default_rng(n))
    assert any(dead) and not all(dead)
    for b, M in enumerate(mats):
        N, piv, is_dead, dmax = R.chol_whiten_ref(G[b], n, R.CHOL_TOL)
        assert sorted(np.nonzero(is_dead)[0].tolist()) == dead[b], (n, b)
        assert np.all(piv[~is_dead] > 1e-4 * dmax), (n, b, piv[~is_dead].min(), dmax)
        assert np.all(np.abs(piv[is_dead]) <= 1e-12 * dmax), (n, b, np.abs(piv[is_dead]).max(), dmax)
        if not dead[b]:
            assert np.linalg.cond(M) <= 1e4, (n, b, np.linalg.cond(M))
            ref = np.linalg.inv(np.linalg.cholesky(M).T)
            assert np.abs(N - ref).max() <= 1e-10 * np.abs(ref).max(), (n, b)
        else:
            live = ~is_dead
            W = N.T @ M @ N
            assert np.abs(W[np.ix_(live, live)] - np.eye(int(live.sum()))).max(initial=0.0) < 1e-10, (n, b)
        # the rule is relative to dmax: with an absolute tolerance the classification of the scaled tiles would differ
        if n >= 7 and b:
            assert not np.array_equal(~(piv > R.CHOL_TOL), is_dead), (n, b)


@functools.lru_cache(maxsize=None)
def _refs(name):
    src = philox.PhiloxSource(R.SEED)
    return R.case_oracles(name, src, R.many_sample() if name == "many" else None)


def test_many_tiles_sample():
    sample = R.many_sample()
    assert len(sample) == R.MANY_SAMPLE == len(set(sample)) and set((0, 4094, 4095)) <= set(sample)
    assert len(R.tiles("many")[1]) == 4225 and max(sample) < max(R.MANY_CALLS)
    for t, by_mode in _refs("many").items():
        assert R.separation(np.linalg.norm(by_mode["f64"].v, axis=1))[2].sum() >= 3, t


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_planted_case_is_admissible(name):
    """Per case, from the float64 oracle and the two fp32 oracles: the components that exist are min(r, bins, pooled
    pixels); enough separated components per tile (MIN_SEPARATED: 30 in A-E, 5 beyond row 64 in C and D, 5 beyond row
    128 in D); the case's own thresholds are the pair with the widest clearance from every statistic of the three
    oracles for which the decisions show a pass after a failure and a cut by max_fail, that clearance is at least five
    knife edges, so no (tile, threshold pair) falls under the knife-edge exemption; the fp32 yardstick is not zero."""
    refs = _refs(name)
    re_ = R.r_eff(name)
    T = R.case_dims(name)[2]
    k_u, k_v, k_sig, k_sp, k_tp, seps = 0.0, 0.0, 0.0, 0.0, 0.0, []
    for t, by_mode in refs.items():
        r64, r32 = by_mode["f64"], by_mode["f32s"]
        assert r64.u.shape[1] == re_ and r64.v.shape == (re_, T) and r64.v_ds.shape == (re_, T) and r64.S.shape == r64.u.shape
        sig = np.linalg.norm(r64.v, axis=1)
        sep = R.separation(sig)[2]
        seps.append((int(sep.sum()), int(sep[64:].sum()), int(sep[128:].sum())))
        s0 = R.block_s0(name, t)
        k_u = max(k_u, R.vector_K(r32.u, r64.u, sig, s0, sep, 0))
        k_v = max(k_v, R.vector_K(r32.v, r64.v, sig, s0, sep, 1))
        k_sig = max(k_sig, R.scalar_K(np.linalg.norm(r32.v, axis=1), sig, sep))
        k_sp = max(k_sp, R.scalar_K(r32.sp, r64.sp, sep))
        k_tp = max(k_tp, R.scalar_K(r32.tp, r64.tp, sep))
        if name == "A":
            # the hook arrays of the staged form: rows of v_ds and columns of S that are compared
            sep_ds = R.separation(r64.s_ds)[2]
            sig_b = np.linalg.svd(r64.v_ds, compute_uv=False)
            sep_b = R.separation(sig_b)[2]
            assert sep_ds.sum() >= 30 and sep_b.sum() >= 30, (t, int(sep_ds.sum()), int(sep_b.sum()))
            assert R.vector_K(r32.v_ds, r64.v_ds, r64.s_ds, r64.s_ds[0], sep_ds, 1) > 0
            assert R.vector_K(r32.S, r64.S, sig_b, sig_b[0], sep_b, 0) > 0
    print(f"\ncase {name}: separated per tile (all, >= 64, >= 128) {seps[:6]}, fp32 yardstick K_U {k_u:.2e} K_V {k_v:.2e} "
          f"sigma {k_sig:.2e} spatial {k_sp:.2e} temporal {k_tp:.2e}")
    if name in R.MIN_SEPARATED:
        need = R.MIN_SEPARATED[name]
        assert all(s[0] >= need[0] and s[1] >= need[1] and s[2] >= need[2] for s in seps), (name, seps)
    assert min(k_u, k_v, k_sig, k_sp, k_tp) > 0
    stats_all, stats64 = R.threshold_stats(refs)
    own, pass_all = R.thresholds(name)
    best, best_c = R.best_thresholds(stats_all, stats64)
    assert best is not None
    # (compared through the clearance, not the pair: two candidates may tie)
    assert min(R.clearance(stats_all, own)) >= (1 - 1e-3) * best_c, (name, own, best, best_c)
    assert min(R.clearance(stats_all, own)) >= MIN_CLEARANCE, (name, R.clearance(stats_all, own))
    assert R.decision_patterns(stats64, own) == {"pass after a failure", "cut by max_fail"}
    knife = sum(not R.margin_ok(sp, tp, thr) for sp, tp in stats_all for thr in (own, pass_all))
    assert knife / (len(stats_all) * 2) <= 0.10


@functools.lru_cache(maxsize=None)
def _degenerate_refs(name):
    return R.case_oracles(name, philox.PhiloxSource(R.SEED))


@pytest.mark.parametrize("name", sorted(R.DEGENERATE))
def test_degenerate_family_is_admissible(name):
    """The tiles of tile_stage_ref.KINDS in the narrow (Zn) and the wide (Zw) case, as conditions on the inputs of
    tests/test_gpu_tile_degenerate.py:
      (a) zero, low3, rank1 and sparse2 hold integers and have exactly rho = 0, 3, 1, 2 nonzero singular values in float64
          (the others below 1e-12 of the first), and so has the pooled, temporally binned tile: pooling hides no component
          from the sketch;
      (b) their nonzero singular values lie within 1e3 of each other, far above the 1e-5 relative whitening cut;
      (c) under the float64 oracle the rho leading components pass the case's thresholds and component rho fails, every
          statistic of these farther than KNIFE_EDGE from its threshold (a NaN statistic fails): the oracle's rank at
          max_fail = 1 is rho + 1.
    The deadrows and live tiles have full rank (72 live pixels / min(pixels, frames)), at least three separated components
    each, a nonzero fp32 yardstick and no strong component of any oracle nearer than KNIFE_EDGE to a threshold."""
    refs = _degenerate_refs(name)
    own = R.thresholds(name)[0]
    (b1, b2), T = R.case_dims(name)[1:]
    d = b1 * b2
    assert R.movie_rows(name).shape == (len(R.KINDS) * d, T) and R.movie_rows(name).dtype == np.float32
    assert np.array_equal(R.tiles(name)[0], np.arange(len(R.KINDS) * d).reshape(len(R.KINDS), d))
    for t, kind in enumerate(R.KINDS):
        X = R.tile_block(name, t).reshape((d, T), order="F").astype(np.float64)
        assert np.array_equal(X, R.movie_rows(name)[t * d:(t + 1) * d])
        r64 = refs[t]["f64"]
        assert r64.u.shape == (d, R.r_eff(name)) and r64.v.shape == (R.r_eff(name), T)
        sv = np.linalg.svd(X, compute_uv=False)
        sv_p = np.linalg.svd(R.pooled_binned(name, t), compute_uv=False)
        if kind in R.RHO:
            rho = R.RHO[kind]
            assert np.array_equal(X, np.round(X)) and np.abs(X).max() * T < 2 ** 24
            for s in (sv, sv_p):
                assert np.all(s[:rho] > 0) and np.all(s[rho:] <= 1e-12 * max(s[0], 1e-300)), (name, kind, s[:rho + 2])
                assert rho == 0 or s[0] <= 1e3 * s[rho - 1], (name, kind, s[:rho])
            sp, tp = r64.sp[:rho + 1], r64.tp[:rho + 1]
            with np.errstate(invalid="ignore"):
                good = (sp < np.float32(own[0])) & (tp < np.float32(own[1]))
            assert good[:rho].all() and not good[rho], (name, kind, sp, tp)
            fin = np.isfinite(sp) & np.isfinite(tp)
            assert fin[:rho].all() and R.margin_ok(sp[fin], tp[fin], own), (name, kind, sp, tp)
            assert R.oracle_rank(r64, own, 1) == rho + 1, (name, kind)
            print(f"\n{name} {kind}: sigma {sv[:rho]}, pooled and binned {sv_p[:rho]}, oracle ranks "
                  f"{[R.oracle_rank(r64, own, mf) for mf in R.MAX_FAILS]}")
        else:
            live_pixels = 72 if kind == "deadrows" else d
            assert np.linalg.matrix_rank(X) == min(live_pixels, T), (name, kind)
            sig = np.linalg.norm(r64.v, axis=1)
            _, strong, sep = R.separation(sig)
            assert sep.sum() >= 3, (name, kind, int(sep.sum()))
            r32 = refs[t]["f32s"]
            s0 = R.block_s0(name, t)
            assert R.vector_K(r32.u, r64.u, sig, s0, sep, 0) > 0 and R.vector_K(r32.v, r64.v, sig, s0, sep, 1) > 0
            for m in R.MODES:
                assert R.margin_ok(refs[t][m].sp[strong], refs[t][m].tp[strong], own), (name, kind, m)
