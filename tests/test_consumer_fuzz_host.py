"""The consumer fuzz on the CPU (tests/consumer_fuzz.py): the frozen draws and their digest, the census of geometry
classes, the two conditions on applies(), the reproducibility of a case, and the checkers themselves: each accepts the
fp64 reference rounded to float32 and rejects the same result with one defect of the kind a kernel would produce."""
import numpy as np
import pytest

from localmd_amd import maps as MP
from tests import consumer_fuzz as F

CASES = F.draw_cases()
HOST_CHECKED = ("export", "traces", "maps", "summary", "quantiles")
DEFECTS = ("ragged_patch", "partial_batch", "roi_pixel")


def test_draws_are_frozen():
    assert F.digest(CASES) == F.DIGEST, F.digest(CASES)
    assert F.digest(F.draw_cases(F.FUZZ_SEED)) == F.DIGEST and F.digest(F.draw_cases(F.FUZZ_SEED + 1)) != F.DIGEST
    assert len(CASES) == 16 and len({c["name"] for c in CASES}) == 16
    for c in CASES:
        small, big = c["fbs"]
        assert 0 < small < c["T"] and c["T"] % small != 0 and big >= c["T"]
        assert c["container"] in ("float32", "uint16")
        assert max(c["d1"], c["d2"]) <= 96 and c["T"] <= 1100
    assert any(c["window"] > c["T"] for c in CASES)
    assert {c["method"] for c in CASES} == {"maximin", "minimum", "percentile"}
    assert {c["summary_bin"] for c in CASES} == {1, 4, 512}


def test_every_class_is_drawn():
    census = {k: [c["name"] for c in CASES if k in F.classes(c)] for k in F.CLASSES}
    for k, names in census.items():
        print(k, len(names), names)
    assert all(census.values()), [k for k, v in census.items() if not v]


def test_applies_leaves_little_out():
    for consumer in F.CONSUMERS:
        run = [c for c in CASES if F.applies(consumer, c) is None]
        assert 4 * len(run) >= 3 * len(CASES), consumer
    for k in F.CLASSES:
        running = [cons for cons in F.CONSUMERS if any(k in F.classes(c) and F.applies(cons, c) is None for c in CASES)]
        assert len(running) >= 6, (k, running)
    for consumer in F.CONSUMERS:
        for c in CASES:
            why = F.applies(consumer, c)
            assert why is None or (isinstance(why, str) and len(why) > 20)
            if why:
                print(consumer, c["name"], ":", why)


@pytest.mark.parametrize("index", [1, 3, 8, 9])
def test_make_case_is_reproducible_and_the_movie_integer_valued(index):
    case = CASES[index]
    pmd, X64, Y = F.make_case(case)
    F._CACHE.clear()
    pmd2, X2, Y2 = F.make_case(case)
    T, d1, d2 = case["T"], case["d1"], case["d2"]
    assert X64.tobytes() == X2.tobytes() and Y.tobytes() == Y2.tobytes() and (pmd.u != pmd2.u).nnz == 0
    assert Y.shape == (T, d1, d2) and Y.dtype == np.float32 and X64.shape == (d1 * d2, T) and X64.dtype == np.float64
    assert np.array_equal(Y, np.rint(Y)) and Y.min() >= 0 and Y.max() <= 65535
    assert np.array_equal(F.container(Y, "uint16").astype(np.float32), Y)
    assert pmd.u.dtype == np.float32 and pmd.r.dtype == np.float32 and pmd.v.dtype == np.float32
    assert pmd.r.shape == (pmd.u.shape[1], case["rank"]) and pmd.v.shape == (case["rank"], T)
    mean, std = np.asarray(pmd.mean_img), np.asarray(pmd.var_img)
    assert mean.min() >= 500 and mean.max() <= 1500 and std.min() >= 2 and std.max() <= 10


def test_the_tile_flags_describe_u():
    for c in CASES:
        u = F.build_u(c)
        n_tile = u.shape[1] - c["K"]
        assert (n_tile > 0) == c["tiles"], c["name"]
        assert u.shape[0] == c["d1"] * c["d2"]
        if c["empty_rows"]:
            assert (np.diff(u.indptr) == 0).any(), c["name"]
        assert len(F.demix_rois(c)) >= 3 and F.demix_rois(c).reshape(len(F.demix_rois(c)), -1).any(axis=1).all()


# ---- the checkers --------------------------------------------------------------------------------------------------
def _movies(case, defect):
    """(X (D, T) float64, Y (T, D) float64 integer-valued): the references, with the defect of a kernel in them."""
    pmd, X64, Y = F.make_case(case)
    T, D = case["T"], case["d1"] * case["d2"]
    X, Yd = X64.copy(), Y.reshape(T, D).astype(np.float64)
    if defect == "ragged_patch":           # the last pixel of the ragged last 64-pixel patch keeps its neighbour's value
        X[D - 1] = X[D - 2]
    if defect == "partial_batch":          # the last frame of the partial last batch is the frame before
        X[:, T - 1] = X[:, T - 2]
        Yd[T - 1] = Yd[T - 2]
    return X, Yd


def _panels32(X, Yd):
    raw, den = Yd.astype(np.float32), X.T.astype(np.float32)
    return {"raw": raw, "denoised": den, "residual": raw - den}


def _three(raw64, den64):
    raw, den = raw64.astype(np.float32), den64.astype(np.float32)
    return {"raw": raw, "denoised": den, "residual": raw - den}


def _numpy_result(consumer, case, defect):
    """What the device would return if it computed in float64 and rounded once, from the (defective) movies."""
    pmd, X64, Y = F.make_case(case)
    T, d1, d2 = case["T"], case["d1"], case["d2"]
    D = d1 * d2
    X, Yd = _movies(case, defect)
    pan = _panels32(X, Yd)
    true = _panels32(X64, Y.reshape(T, D).astype(np.float64))
    if consumer == "export":
        f = np.concatenate([pan[p].reshape(T, d1, d2) for p in case["panels"]], axis=2)
        return {"f32": f, "int": F.quantize(f, case["out_dtype"])}
    if consumer == "traces":
        lab, values = F.roi_labels(case)
        out = {}
        for name, w, reduce in (("bool_sum", F.roi_masks(case), "sum"), ("float_sum", F.roi_weights_of(case), "sum"),
                                ("float_mean", F.roi_weights_of(case), "mean"),
                                ("label", np.stack([lab == v for v in values]), "mean")):
            W = F.w64(w, reduce)
            if defect == "roi_pixel":      # the first ROI loses its last pixel
                W = W.copy()
                W[0, np.nonzero(W[0])[0][-1]] = 0.0
            K = len(W)
            out[name] = {k: v.reshape(K, T) for k, v in _three(W @ Yd.T, W @ X).items()}
        out["stack"] = out["label"]
        return out
    if consumer == "maps":
        R = F.regressors(case)
        sx = R.sum(axis=1)[:, None]
        out = {"sum": {k: v.reshape(-1, d1, d2) for k, v in _three(R @ Yd, R @ X.T).items()},
               "mean": {k: v.reshape(-1, d1, d2) for k, v in _three(R @ Yd / sx, R @ X.T / sx).items()}}
        xhat = MP.normalized_regressors(F.corr_regressors(case)).astype(np.float32).astype(np.float64)
        Z = F.centred_panels(pmd, pan, Yd.astype(np.float32).reshape(T, d1, d2))
        out["correlation"] = {}
        for kind in F.ALL:
            r, kappa = F.pearson64(xhat, Z[kind])
            out["correlation"][kind] = np.where(np.isfinite(kappa)[None, :], r, 0.0).astype(np.float32).reshape(-1, d1, d2)
        out["exported"] = true
        return out
    if consumer == "summary":
        noise = np.asarray(pmd.var_img, np.float64).reshape(-1)
        vals = {k: pan[k].astype(np.float64) for k in F.ALL}          # the float32 frames the kernel sums
        out = {"exported": true}
        for kind in F.ALL:
            lo, hi, alo, ahi = F.binned_extrema(pan[kind], case["summary_bin"])
            v = vals[kind]
            mean = v.mean(axis=0)
            d = v - mean
            m2, m3, m4 = ((d ** p).mean(axis=0) for p in (2, 3, 4))
            m3, m4, m2 = np.where(m2 > 0, m3, 0.0), np.where(m2 > 0, m4, 3.0), np.where(m2 > 0, m2, 1.0)   # constant: 0, 0, 0
            img = {"min": lo, "max": hi, "argmin": alo, "argmax": ahi, "mean": mean, "std": np.sqrt(np.where(np.ptp(v, axis=0) > 0, m2, 0.0)),
                   "skewness": m3 / m2 ** 1.5, "kurtosis": m4 / m2 ** 2 - 3.0, "pnr": (hi.astype(np.float64) - mean) / noise}
            out[kind] = {k: a.reshape(d1, d2).astype(np.int32 if k.startswith("arg") else np.float32) for k, a in img.items()}
        return out
    if consumer == "quantiles":
        out = {"exported": true, "q": {}, "mad": {}}
        for kind in F.ALL:
            S = np.sort(pan[kind], axis=0)
            out["q"][kind] = F.quantile_reference(S, F.quantiles_of(case), "linear").reshape(-1, d1, d2)
            out["mad"][kind] = F.mad_reference(pan[kind], S).reshape(d1, d2)
        return out
    raise AssertionError(consumer)


def _host_case(index):
    """The case with all three panels exported, so that every defect is in view of check_export."""
    return dict(CASES[index], panels=F.TRIPTYCH)


@pytest.mark.parametrize("index", [3, 7])
@pytest.mark.parametrize("consumer", HOST_CHECKED)
def test_checker_accepts_the_rounded_reference(consumer, index):
    case = _host_case(index)
    figures = {}
    F.CHECK[consumer](_numpy_result(consumer, case, None), case, figures)
    print(consumer, case["name"], figures)
    assert all(v <= 1.0 for v in figures.values())


@pytest.mark.parametrize("index", [3, 7])
@pytest.mark.parametrize("consumer,defect", [(c, d) for c in HOST_CHECKED for d in DEFECTS
                                             if d != "roi_pixel" or c == "traces"])      # only extract_traces holds ROIs
def test_checker_rejects_one_defect(consumer, defect, index):
    case = _host_case(index)
    with pytest.raises(AssertionError):
        F.CHECK[consumer](_numpy_result(consumer, case, defect), case)
