"""Seeded fuzz of the PMDArray consumers over field-of-view and tile geometry (holds no test): the frozen draws, the
geometry classes they cover, the synthetic case of a draw, which (consumer, case) pairs are run, one runner and one checker
per consumer, and the bounds and references the consumers' own GPU modules apply to their one fixture, here with the
field of view and the length as parameters (those modules import them from here).

A case is a synthetic PMDArray, not a decomposition: U from _random_tiled_u, random R, s, Vt, mean in [500, 1500], std in
[2, 10].  The fp64 reference of every consumer is formed from the factors: X64 = mean + std * (U (R diag(s)) Vt) with U in C
pixel order; the raw movie Y is X64 plus noise and a few planted discs, rounded to integers within uint16 and held as
float32, so its float32 and uint16 containers hold the same values.

tests/test_consumer_fuzz_host.py checks the draws, the census and the checkers on the CPU; tests/test_gpu_consumer_fuzz.py
runs every pair on the device."""
import hashlib

import numpy as np

from tests import baseline_quantile_ref as BQ
from tests import baseline_ref as BR
from tests.test_export_host import _random_tiled_u
from tests.test_traces_host import _disc

U24 = 2.0 ** -24
GAMMA = 1032 * U24                     # maps.GAMMA: any order of <= 1024 fp32 terms plus the roundings of the operands
ALL = ("denoised", "raw", "residual")
TRIPTYCH = ("raw", "denoised", "residual")
CONSUMERS = ("export", "traces", "maps", "summary", "quantiles", "baseline", "project", "superpixels", "demix", "grow")
MOMENTS = ("mean", "std", "skewness", "kurtosis")
EXTREMA = ("min", "max", "argmin", "argmax")
FUZZ_SEED = 20
DIGEST = "af42bc6cdfb25f66"            # of draw_cases(FUZZ_SEED): an edit to the draw code shows up here


# ---- the draws -----------------------------------------------------------------------------------------------------
# (d1, d2, b1, b2, order, K, tiles, merged, empty_rows, rank, T): the geometry of every draw is pinned, so that every class
# of classes() is met whatever the seed; the seed draws everything else.  tiles=False: U holds the K background columns
# only (b1, b2 then say nothing).
_GEOMETRY = (
    (40, 44, 20, 20, "F", 2, True, False, False, 6, 600),
    (1, 65, 1, 16, "C", 1, True, False, False, 4, 300),             # one row; D % 64 == 1; tiles of 16 pixels
    (64, 1, 16, 1, "F", 1, True, False, False, 3, 257),             # one column; D % 64 == 0
    (7, 9, 7, 9, "F", 0, True, False, False, 1, 100),               # D = 63 < 64: one ragged patch; one tile; rank 1
    (31, 37, 10, 8, "C", 2, True, True, True, 5, 1023),
    (32, 32, 16, 16, "F", 0, True, False, False, 6, 1024),          # no background column
    (65, 65, 20, 22, "C", 1, True, True, False, 8, 1025),           # D % 64 == 1
    (15, 17, 6, 8, "F", 1, True, False, True, 4, 513),              # D % 64 == 63; tiles of 48 pixels
    (45, 50, 20, 20, "C", 3, False, False, False, 3, 400),          # background columns only
    (23, 37, 10, 10, "F", 0, False, False, False, 2, 300),          # no column at all
    (48, 40, 24, 20, "F", 1, True, False, False, 1, 700),           # rank 1
    (96, 96, 32, 32, "C", 2, True, False, False, 12, 1100),         # the largest
    (20, 24, 20, 24, "C", 0, True, False, False, 3, 37),            # one tile, fewer frames than anything is sliced by
    (50, 30, 25, 10, "F", 0, True, True, False, 5, 640),
    (72, 81, 24, 27, "F", 1, True, False, True, 7, 900),
    (3, 70, 3, 10, "C", 2, True, True, False, 4, 333),              # tiles of 30 pixels
)
_PANEL_SETS = (("denoised",), ("raw",), ("residual",), ("raw", "denoised"), ("denoised", "residual"), ("residual", "raw"),
               TRIPTYCH)


def draw_cases(seed=FUZZ_SEED):
    """The list of cases (dicts) of ``seed``.  Beside the geometry: ``seed`` (of the factors and the movie), ``fbs`` (two
    frame batch sizes: one below T that does not divide it, one of at least T), ``container`` (of the raw movie), and
    what the consumers draw: the panels and element type of the export, the temporal bin of the summary, a quantile, the
    bin, window, method, q and output of the baseline."""
    rng = np.random.default_rng(seed)
    out = []
    for i, (d1, d2, b1, b2, order, K, tiles, merged, empty_rows, rank, T) in enumerate(_GEOMETRY):
        small = int(rng.integers(max(2, T // 6), T))
        while T % small == 0:
            small -= 1
        method = ("maximin", "minimum", "percentile")[i % 3]
        base_bin = int(rng.choice([4, 16, 64] if method == "percentile" else [1, 4, 16, 256]))
        window = int(rng.integers(5, max(6, T // 2)))
        if i == 2:
            window = T + int(rng.integers(1, 200))                   # a window beyond the movie
        c = dict(index=i, d1=d1, d2=d2, b1=b1, b2=b2, order=order, K=K, tiles=tiles, merged=merged, empty_rows=empty_rows,
                 rank=rank, T=T, seed=int(rng.integers(1, 2 ** 31)), fbs=(small, T + int(rng.integers(0, 500))),
                 container=str(rng.choice(["float32", "uint16"])),
                 panels=_PANEL_SETS[int(rng.integers(len(_PANEL_SETS)))], out_dtype=str(rng.choice(["uint16", "int16"])),
                 summary_bin=int(rng.choice([1, 4, 512])), q=round(float(rng.uniform(0.02, 0.98)), 3),
                 base_bin=base_bin, window=window, method=method, base_q=round(float(rng.uniform(0.05, 0.6)), 2),
                 output=str(rng.choice(["dff", "detrended", "baseline"])))
        c["name"] = "{}-{}x{}{}-b{}x{}-K{}-r{}-T{}{}{}".format(
            i, d1, d2, order, *((b1, b2) if tiles else ("-", "-")), K, rank, T, "-merged" if merged else "",
            "-emptyrows" if empty_rows else "")
        out.append(c)
    return out


def digest(cases):
    return hashlib.sha256(repr([sorted(c.items()) for c in cases]).encode()).hexdigest()[:16]


CLASSES = ("D%64==0", "D%64==1", "D%64==63", "D<64", "d1==1", "d2==1", "single tile", "tile<64px", "merged", "empty_rows",
           "K==0 with tiles", "background only", "no column", "rank==1", "T<256", "T==1023", "T==1024", "T==1025",
           "order F", "order C")


def classes(case):
    """The geometry classes of CLASSES the case belongs to."""
    D, c = case["d1"] * case["d2"], case
    is_in = {"D%64==0": D % 64 == 0, "D%64==1": D % 64 == 1, "D%64==63": D % 64 == 63, "D<64": D < 64,
             "d1==1": c["d1"] == 1, "d2==1": c["d2"] == 1,
             "single tile": c["tiles"] and c["b1"] == c["d1"] and c["b2"] == c["d2"],
             "tile<64px": c["tiles"] and c["b1"] * c["b2"] < 64, "merged": c["tiles"] and c["merged"],
             "empty_rows": c["empty_rows"], "K==0 with tiles": c["tiles"] and c["K"] == 0,
             "background only": not c["tiles"] and c["K"] > 0, "no column": not c["tiles"] and c["K"] == 0,
             "rank==1": c["rank"] == 1, "T<256": c["T"] < 256, "T==1023": c["T"] == 1023, "T==1024": c["T"] == 1024,
             "T==1025": c["T"] == 1025, "order F": c["order"] == "F", "order C": c["order"] == "C"}
    assert tuple(is_in) == CLASSES
    return tuple(k for k in CLASSES if is_in[k])


def applies(consumer, case):
    """None when ``consumer`` runs on ``case``, else the reason it does not: a pure function of the geometry, and the only
    way a pair is left out."""
    assert consumer in CONSUMERS
    if not case["tiles"] and case["K"] == 0 and consumer in ("superpixels", "demix", "grow"):
        return ("U has no column: the denoised movie is the mean image in every frame, so no pixel correlates with any "
                "other and there is nothing to segment, demix or grow")
    return None


# ---- a case --------------------------------------------------------------------------------------------------------
_CACHE = {}


def build_u(case):
    c = case
    b1, b2 = (c["b1"], c["b2"]) if c["tiles"] else (c["d1"] + 1, c["d2"] + 1)       # no tile fits: background only
    return _random_tiled_u(c["d1"], c["d2"], b1, b2, c["order"], c["K"], c["seed"] % 10 ** 6, merged=c["merged"],
                           empty_rows=c["empty_rows"]).astype(np.float32)


def planted(case):
    """(masks (n, d1, d2) bool, traces (n, T)): a few discs with sparse decaying events, added to the raw movie."""
    d1, d2, T = case["d1"], case["d2"], case["T"]
    rng = np.random.default_rng([case["seed"], 1])
    n = 3
    masks = np.stack([_disc(d1, d2, int(rng.integers(0, d1)), int(rng.integers(0, d2)), float(rng.uniform(1.5, 4.5)))
                      for _ in range(n)])
    traces = np.zeros((n, T))
    for k in range(n):
        for t0 in rng.choice(T, max(2, T // 40), replace=False):
            m = min(20, T - t0)
            traces[k, t0:t0 + m] += rng.uniform(20, 60) * np.exp(-np.arange(m) / 5.0)
    return masks, traces


def make_case(case):
    """(pmd, X64, Y): the PMDArray with float32 factors, the dense fp64 movie (D, T) with pixels in C order, and the raw
    movie (T, d1, d2), integer-valued float32 within uint16.  Cached by the case's name; treat all three as read-only."""
    from localmd_amd.pmdarray import PMDArray

    if case["name"] in _CACHE:
        return _CACHE[case["name"]]
    d1, d2, T, rank = case["d1"], case["d2"], case["T"], case["rank"]
    D = d1 * d2
    u = build_u(case)
    rng = np.random.default_rng([case["seed"], 0])
    k = u.shape[1]
    f32 = np.float32
    pmd = PMDArray(u, (rng.standard_normal((k, rank)) * 0.1).astype(f32), np.linspace(20, 2, rank).astype(f32),
                   (rng.standard_normal((rank, T)) * 0.05 + rng.uniform(-0.02, 0.02, (rank, 1))).astype(f32), (T, d1, d2),
                   case["order"], rng.uniform(500, 1500, (d1, d2)).astype(f32), rng.uniform(2, 10, (d1, d2)).astype(f32))
    X64 = den64(pmd, absolute=False)
    masks, traces = planted(case)
    std = np.asarray(pmd.var_img, np.float64).reshape(-1)
    noise = std[:, None] * rng.standard_normal((D, T)) + masks.reshape(len(masks), D).T.astype(np.float64) @ traces
    Y = np.clip(np.rint(X64 + noise), 0, 65535).T.reshape(T, d1, d2).astype(f32)
    _CACHE[case["name"]] = (pmd, X64, Y)
    return _CACHE[case["name"]]


def container(Y, name):
    return Y if name == "float32" else Y.astype(name)


# ---- fp64 references from the factors --------------------------------------------------------------------------------
def factors64(pmd):
    """(mean, std, U in C pixel order, R diag(s), Vt) in float64."""
    uc = pmd.u.astype(np.float64).toarray()[pmd.row_indices.reshape(-1)]
    rs = pmd.r.astype(np.float64) * pmd.s.astype(np.float64)[None, :]
    return (np.asarray(pmd.mean_img, np.float64).reshape(-1), np.asarray(pmd.var_img, np.float64).reshape(-1), uc, rs,
            pmd.v.astype(np.float64))


def den64(pmd, absolute=True):
    """(X64, |X| bound) of the denoised movie, (D, T) float64, pixels in C order; X64 alone with absolute=False."""
    mean, std, uc, rs, vt = factors64(pmd)
    X = mean[:, None] + std[:, None] * (uc @ rs @ vt)
    if not absolute:
        return X
    return X, np.abs(mean)[:, None] + std[:, None] * (np.abs(uc) @ np.abs(rs) @ np.abs(vt))


def recon64(pmd):
    """The denoised movie (T, d1, d2) float64."""
    d1, d2 = pmd.shape[1:]
    return np.ascontiguousarray(den64(pmd, absolute=False).T).reshape(-1, d1, d2)


def rel(got, want):
    """The largest difference relative to the largest reference value."""
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def den_bound(absX):
    """The forward bound of an expanded denoised value (test_gpu_export.test_kernel_against_fp64, and of its weighted sums
    in test_gpu_traces / test_gpu_maps): 1e-5 of the sum of magnitudes plus 1e-6."""
    return 1e-5 * absX + 1e-6


def panels_of(a, panels, d2):
    """{panel: (T, D) contiguous} of a (T, d1, len(panels) d2) export."""
    T = a.shape[0]
    return {p: np.ascontiguousarray(a[:, :, j * d2:(j + 1) * d2]).reshape(T, -1) for j, p in enumerate(panels)}


def exported(ctx, pmd, mov):
    """{kind: (T, D) float32} of export_movie, the fp32 frames the per-pixel kernels see."""
    import localmd_amd

    T, d1, d2 = (int(x) for x in pmd.shape)
    out = np.empty((T, d1, 3 * d2), np.float32)
    localmd_amd.export_movie(pmd, out, mov, panels=TRIPTYCH, dtype="float32", ctx=ctx)
    return panels_of(out, TRIPTYCH, d2)


# ---- traces ---------------------------------------------------------------------------------------------------------
def w64(w, reduce):
    W = w.reshape(w.shape[0], -1).astype(np.float64)
    return W / W.sum(axis=1, keepdims=True) if reduce == "mean" else W


def raw_bound(W64, Y64):
    """(p + 4) 2^-24 (|W| |Y|): one rounding per product and per addition of a p-term chain plus the segment adds,
    plus the weight's own rounding."""
    p = (W64 != 0).sum(axis=1)
    return (p + 4)[:, None] * U24 * (np.abs(W64) @ np.abs(Y64))


def roi_masks(case):
    """(K, d1, d2) bool: a few random discs, a one-pixel ROI at the last pixel, the whole field."""
    d1, d2 = case["d1"], case["d2"]
    rng = np.random.default_rng([case["seed"], 2])
    m = [_disc(d1, d2, int(rng.integers(0, d1)), int(rng.integers(0, d2)), float(rng.uniform(1.0, 6.0))) for _ in range(4)]
    one = np.zeros((d1, d2), bool)
    one[d1 - 1, d2 - 1] = True
    return np.stack(m + [one, np.ones((d1, d2), bool)])


def roi_weights_of(case):
    """roi_masks with weights that are not exactly representable in fp32."""
    m = roi_masks(case)
    return m * np.random.default_rng([case["seed"], 3]).uniform(0.1, 2.0, m.shape)


def roi_labels(case):
    """(label image, its labels ascending): the masks painted one over the other, so they no longer overlap."""
    m = roi_masks(case)
    lab = np.zeros(m.shape[1:], np.int64)
    for k in (5, 0, 1, 2, 3, 4):                       # the whole field first
        lab[m[k]] = 3 * k + 2
    return lab, np.unique(lab)


def _kinds(tr):
    return {k: getattr(tr, k) for k in ALL}


def run_traces(ctx, case, movie, fbs, resident=False):
    import localmd_amd

    pmd = make_case(case)[0]
    kw = dict(kinds=ALL, frame_batch_size=fbs, **({} if resident else {"ctx": ctx}))
    lab, values = roi_labels(case)
    return {"bool_sum": _kinds(localmd_amd.extract_traces(pmd, roi_masks(case), movie, reduce="sum", **kw)),
            "float_sum": _kinds(localmd_amd.extract_traces(pmd, roi_weights_of(case), movie, reduce="sum", **kw)),
            "float_mean": _kinds(localmd_amd.extract_traces(pmd, roi_weights_of(case), movie, reduce="mean", **kw)),
            "label": _kinds(localmd_amd.extract_traces(pmd, lab, movie, reduce="mean", **kw)),
            "stack": _kinds(localmd_amd.extract_traces(pmd, np.stack([lab == v for v in values]), movie, reduce="mean", **kw))}


def traces_ratios(tr, W64, Y64, X64, absX):
    """(raw error / raw_bound, denoised error / den_bound), the largest of each."""
    rb, db = raw_bound(W64, Y64), den_bound(np.abs(W64) @ absX)
    return float((np.abs(tr["raw"] - W64 @ Y64) / rb).max()), float((np.abs(tr["denoised"] - W64 @ X64) / db).max())


def check_traces(result, case, figures=None):
    pmd, X64, Y = make_case(case)
    T, D = case["T"], case["d1"] * case["d2"]
    Y64 = Y.reshape(T, D).astype(np.float64).T
    absX = den64(pmd)[1]
    masks = roi_masks(case)
    lab, values = roi_labels(case)
    worst = [0.0, 0.0]
    for name, w, reduce in (("bool_sum", masks, "sum"), ("float_sum", roi_weights_of(case), "sum"),
                            ("float_mean", roi_weights_of(case), "mean"),
                            ("label", np.stack([lab == v for v in values]), "mean")):
        tr, W64 = result[name], w64(w, reduce)
        for a in tr.values():
            assert a.shape == (len(w), T) and a.dtype == np.float32, name
        if name == "bool_sum":                          # boolean masks under "sum": every partial sum is an integer
            assert D * np.abs(Y64).max() < 2 ** 24
            assert np.array_equal(tr["raw"].astype(np.float64), W64 @ Y64), name
        r, d = traces_ratios(tr, W64, Y64, X64, absX)
        worst = [max(worst[0], r), max(worst[1], d)]
        assert r <= 1.0, (name, "raw", r)
        assert d <= 1.0, (name, "denoised", d)
        assert np.array_equal(tr["residual"], tr["raw"] - tr["denoised"]), name
    assert bytes_of(result["label"]) == bytes_of(result["stack"])
    if figures is not None:
        figures.update({"raw": worst[0], "denoised": worst[1]})


# ---- export ---------------------------------------------------------------------------------------------------------
def quantize(v, dtype):
    """Round half to even, saturate, NaN -> 0 (tests/register_ref.quantize states it)."""
    from tests.register_ref import quantize as q

    return q(v, dtype)


def getitem_frames(case):
    T = case["T"]
    return sorted({0, T // 3, T - 1})


def run_export(ctx, case, movie, fbs, resident=False):
    import localmd_amd

    pmd = make_case(case)[0]
    T, d1, d2, panels = case["T"], case["d1"], case["d2"], case["panels"]
    kw = dict(panels=panels, frame_batch_size=fbs, **({} if resident else {"ctx": ctx}))
    mv = movie if set(panels) != {"denoised"} else None
    f = np.full((T, d1, len(panels) * d2), np.nan, np.float32)
    localmd_amd.export_movie(pmd, f, mv, dtype="float32", **kw)
    q = np.zeros(f.shape, np.dtype(case["out_dtype"]))
    localmd_amd.export_movie(pmd, q, mv, dtype=case["out_dtype"], **kw)
    out = {"f32": f, "int": q}
    if resident:
        out["getitem"] = np.asarray(pmd[getitem_frames(case)], np.float32)
    return out


def check_export(result, case, figures=None):
    pmd, X64, Y = make_case(case)
    T, d1, d2, panels = case["T"], case["d1"], case["d2"], case["panels"]
    bound = den_bound(den64(pmd)[1]).T                                                # (T, D)
    y32, x64 = Y.reshape(T, -1), X64.T
    got = result["f32"]
    assert got.shape == (T, d1, len(panels) * d2) and got.dtype == np.float32
    pan = panels_of(got, panels, d2)
    worst = 0.0
    if "raw" in pan:
        assert np.array_equal(pan["raw"], y32)
    if "denoised" in pan:
        worst = float((np.abs(pan["denoised"] - x64) / bound).max())
        assert worst <= 1.0, ("denoised", worst)
        if "residual" in pan:
            assert np.array_equal(pan["residual"], y32 - pan["denoised"])            # from the rounded denoised panel
    if "residual" in pan:
        rb = bound + 1e-4 * np.abs(y32)
        ratio = float((np.abs(pan["residual"] - (y32 - x64)) / rb).max())
        assert ratio <= 1.0, ("residual", ratio)
    assert result["int"].dtype == np.dtype(case["out_dtype"])
    assert np.array_equal(result["int"], quantize(got, case["out_dtype"]))
    if "getitem" in result and ("denoised" in pan or "exported" in result):
        # pmd[...] after to_device(), with the tolerance of test_gpu_parity.test_pmdarray_device_expansion_matches_host
        h = result.get("exported", pan)["denoised"][getitem_frames(case)].reshape(-1, d1, d2)
        g = result["getitem"]
        assert g.shape == h.squeeze().shape and g.dtype == np.float32          # __getitem__ squeezes a one-pixel-wide field
        np.testing.assert_allclose(g, h.squeeze(), rtol=2e-5, atol=2e-5 * max(1.0, float(np.abs(h).max())))
    if figures is not None:
        figures["denoised"] = worst


# ---- maps -----------------------------------------------------------------------------------------------------------
def sum_bounds(X64, Y64, X64den, absX, mean32):
    """(raw64, raw bound, den64, den bound) of the "sum" maps, (K, D) float64.  The raw bound is the one the feature was
    specified with, in terms of the mean image, and is kept in that form although the device centres by
    maps.centring_vector (the mean rounded to a dyadic grid, within std / 16 of it): a bound in the device's own
    centring would follow the implementation, this one is independent of it."""
    raw64 = X64 @ Y64
    rb = GAMMA * (np.abs(X64) @ np.abs(Y64 - mean32[None, :])) + 2.0 ** -22 * np.abs(raw64)
    d64 = X64 @ X64den.T
    db = 1e-5 * (np.abs(X64) @ absX.T) + 1e-6
    return raw64, rb, d64, db


def check_sums(m, X64, Y64, X64den, absX, mean32, stat, d1, d2, figures=None):
    """``m``: an object or dict with denoised / raw / residual (K, d1, d2) float32 maps of stat "sum" or "mean"."""
    get = m.get if isinstance(m, dict) else (lambda k: getattr(m, k))
    D = d1 * d2
    raw64, rb, d64, db = sum_bounds(X64, Y64, X64den, absX, mean32)
    if stat == "mean":
        sx = X64.sum(axis=1)[:, None]
        raw64, d64 = raw64 / sx, d64 / sx
        rb = GAMMA * (np.abs(X64) @ np.abs(Y64 - mean32[None, :])) / np.abs(sx) + 2.0 ** -22 * np.abs(raw64)
        db = 1e-5 * (np.abs(X64) @ absX.T) / np.abs(sx) + 1e-6
    K = X64.shape[0]
    for k in ALL:
        assert get(k).shape == (K, d1, d2) and get(k).dtype == np.float32
    er, ed = np.abs(get("raw").reshape(K, D) - raw64), np.abs(get("denoised").reshape(K, D) - d64)
    print(stat, "raw: max error / bound", (er / rb).max(), "denoised:", (ed / db).max())
    if figures is not None:
        figures[stat + " raw"], figures[stat + " denoised"] = float((er / rb).max()), float((ed / db).max())
    assert np.all(er <= rb)
    assert np.all(ed <= db)
    assert np.array_equal(get("residual"), get("raw") - get("denoised"))


def pearson64(x, Z):
    """(r, kappa): float64 Pearson correlation of the rows of x (K, T) with the columns of Z (T, P), and
    kappa_p = |z_p| / |z_p - mean z_p|."""
    xc = x - x.mean(axis=1, keepdims=True)
    zc = Z - Z.mean(axis=0, keepdims=True)
    nz = np.sqrt((zc * zc).sum(axis=0))
    with np.errstate(divide="ignore", invalid="ignore"):       # a pixel without variance: r is NaN, kappa infinite
        r = (xc @ zc) / (np.sqrt((xc * xc).sum(axis=1))[:, None] * nz[None, :])
        return r, np.sqrt((Z * Z).sum(axis=0)) / nz


def corr_bound(kappa):
    """Forward bound of the device correlation against the float64 Pearson correlation of the same fp32-valued inputs,
    from the bounds of the kernel test: with g = GAMMA = 1032 2^-24 every block sum is known to g times its sum of
    magnitudes, so, by Cauchy-Schwarz and |x^| = 1,
        |d S_xz| <= g |x^| |z| = g |z|,  |d S_z| <= g sqrt(T) |z|,  |d S_zz| <= g |z|^2.
    With s_z = |z - mean z| = |z| / kappa the numerator N = S_xz - S_x S_z / T (|S_x| <= T 2^-25 max |x^| for the rounded,
    centred x^: its term is of second order) is off by g |z|, which is g kappa in r.  The variance V = S_zz - S_z^2 / T is
    off by |d S_zz| + 2 |S_z| |d S_z| / T <= g |z|^2 (1 + 2 sqrt(1 - kappa^-2)), since |S_z| / sqrt(T) = |mean z| sqrt(T) =
    |z| sqrt(1 - kappa^-2); relative to V = |z|^2 / kappa^2 and halved by the square root that is
    g kappa^2 (1/2 + sqrt(1 - kappa^-2)) in r (|r| <= 1).  Together
        |r - r64| <= g kappa + g kappa^2 (1/2 + sqrt(1 - kappa^-2)) + 2^-23,
    the last term covering the one rounding to float32 (2^-25) and the terms of second order in g.  For every kappa this
    is at most 2.5 g kappa^2; near kappa = 1, as on a movie about its centring vector, it is about 1.6 g."""
    return GAMMA * kappa + GAMMA * kappa * kappa * (0.5 + np.sqrt(np.maximum(0.0, 1.0 - kappa ** -2.0))) + 2.0 ** -23


def regressors(case):
    """(4, T) float64: three random time courses, one of them on an offset near 900, and a row of ones."""
    X = np.random.default_rng([case["seed"], 4]).standard_normal((4, case["T"]))
    X[2] += 900.0
    X[3] = 1.0
    return X


def corr_regressors(case):
    """The first three rows: a constant regressor correlates with nothing, test_gpu_maps covers it."""
    return regressors(case)[:3]


def run_maps(ctx, case, movie, fbs, resident=False):
    import localmd_amd

    pmd = make_case(case)[0]
    kw = dict(kinds=ALL, frame_batch_size=fbs, **({} if resident else {"ctx": ctx}))
    out = {stat: _kinds(localmd_amd.regressor_maps(pmd, regressors(case), movie, stat=stat, **kw)) for stat in ("sum", "mean")}
    out["correlation"] = _kinds(localmd_amd.regressor_maps(pmd, corr_regressors(case), movie, stat="correlation", **kw))
    return out


def check_correlation(m, xhat, Z, d1, d2, figures=None):
    """``m``: {kind: (K, d1, d2) float32}; ``xhat``: the normalised regressors as the device holds them (fp32 values in
    float64); ``Z``: {kind: (T, D) float64}, the fp32 values the kernel correlates."""
    D, K = d1 * d2, len(xhat)
    for kind in ALL:
        got = m[kind]
        assert got.shape == (K, d1, d2) and got.dtype == np.float32
        r64, kappa = pearson64(xhat, Z[kind])
        var = np.isfinite(kappa)                                 # pixels whose fp32 values vary at all
        assert np.all(got.reshape(K, D)[:, ~var] == 0), kind
        if kind == "raw":
            assert var.sum() > 0.9 * D
        if var.any():
            bound = corr_bound(kappa[var])[None, :]
            err = np.abs(got.reshape(K, D)[:, var] - r64[:, var])
            print(kind, "kappa max", kappa[var].max(), "max error / bound", (err / bound).max())
            if figures is not None:
                figures["correlation " + kind] = float((err / bound).max())
            assert np.all(err <= bound), kind
        assert np.all(np.abs(got) <= 1.0)


def centred_panels(pmd, panels, Y):
    """{kind: (T, D) float64}: what the correlation kernel sees: the raw frames minus the centring vector, the expanded
    denoised frames minus the mean image, and the expanded residual frames."""
    from localmd_amd import maps as MP

    T = Y.shape[0]
    mean32 = np.asarray(pmd.mean_img, np.float32).reshape(-1)
    return {"raw": (Y.reshape(T, -1) - MP.centring_vector(pmd)[None, :]).astype(np.float64),
            "denoised": (panels["denoised"] - mean32[None, :]).astype(np.float64),
            "residual": panels["residual"].astype(np.float64)}


def check_maps(result, case, figures=None):
    """result: the three stats, and ``exported``, the float32 panels of export_movie."""
    from localmd_amd import maps as MP

    pmd, X64, Y = make_case(case)
    T, d1, d2 = case["T"], case["d1"], case["d2"]
    Y64 = Y.reshape(T, -1).astype(np.float64)
    absX = den64(pmd)[1]
    mean32 = np.asarray(pmd.mean_img, np.float32).reshape(-1).astype(np.float64)
    for stat in ("sum", "mean"):
        check_sums(result[stat], regressors(case), Y64, X64, absX, mean32, stat, d1, d2, figures)
    xhat = MP.normalized_regressors(corr_regressors(case)).astype(np.float32).astype(np.float64)
    check_correlation(result["correlation"], xhat, centred_panels(pmd, result["exported"], Y), d1, d2, figures)


# ---- summary --------------------------------------------------------------------------------------------------------
def binned_extrema(Yk, bin, block=1024):
    """(min, max, argmin, argmax) of the binned series of the (T, D) float32 movie: per block of 1024 frames the values
    of test_summary_host.emulate_bins (for bin == 1 the frames themselves), first occurrences, frame numbers."""
    from tests.test_summary_host import emulate_bins

    starts, vals = [], []
    for c0 in range(0, len(Yk), block):
        s, v = emulate_bins(Yk[c0:c0 + block], bin)
        starts.append(c0 + s)
        vals.append(v)
    starts, v = np.concatenate(starts), np.concatenate(vals)
    return v.min(axis=0), v.max(axis=0), starts[v.argmin(axis=0)].astype(np.int32), starts[v.argmax(axis=0)].astype(np.int32)


def extrema_equal_export(s, panels, d1, d2, temporal_bin=1):
    """The extrema of every kind of ``s`` ({kind: {stat: image}}) and the frames that attain them are those of the
    exported float32 movie ``panels``, bit for bit."""
    for kind in ALL:
        img, Yk = s[kind], panels[kind]
        for k in ("min", "max"):
            assert img[k].shape == (d1, d2) and img[k].dtype == np.float32
            assert img["arg" + k].shape == (d1, d2) and img["arg" + k].dtype == np.int32
        if temporal_bin == 1:
            lo, hi, alo, ahi = Yk.min(axis=0), Yk.max(axis=0), Yk.argmin(axis=0), Yk.argmax(axis=0)
        else:
            lo, hi, alo, ahi = binned_extrema(Yk, temporal_bin)
        assert img["min"].tobytes() == lo.tobytes() and img["max"].tobytes() == hi.tobytes(), kind
        assert np.array_equal(img["argmin"].reshape(-1), alo), kind
        assert np.array_equal(img["argmax"].reshape(-1), ahi), kind


def _powers(Z):
    """(Z, Z^2, Z^3, Z^4) by products (NumPy's ** goes through pow() for the last two)."""
    z2 = Z * Z
    return Z, z2, z2 * Z, z2 * z2


def moment_bounds(Z):
    """(reference, bound) per stat for the (T, N) float64 values Z = y - centre (the mean is that of Z; add the centre).

    The kernel bound (test_gpu_summary.test_kernel_float_data_within_the_forward_bound), summed over the blocks: the device
    sums S_p are within g A_p of the exact ones, g = GAMMA, A_p = sum |z|^p.  With a_p = S_p / T, alpha_p = A_p / T the
    finishing formulas of summary.finish_moments give, to first order in g,
        mean  = centre + a_1:                          |d mean| <= g alpha_1
        m_2   = a_2 - a_1^2:                           |d m_2| <= e_2 = g (alpha_2 + 2 |a_1| alpha_1)
        m_3   = a_3 - 3 a_1 a_2 + 2 a_1^3:             |d m_3| <= e_3 = g (alpha_3 + 3 |a_1| alpha_2 + (3 |a_2| + 6 a_1^2) alpha_1)
        m_4   = a_4 - 4 a_1 a_3 + 6 a_1^2 a_2 - 3 a_1^4:
                |d m_4| <= e_4 = g (alpha_4 + 4 |a_1| alpha_3 + 6 a_1^2 alpha_2 + (4 |a_3| + 12 |a_1| |a_2| + 12 |a_1|^3) alpha_1)
        std   = m_2^(1/2):                             |d std|  <= e_2 / (2 std)
        skew  = m_3 m_2^(-3/2):                        |d skew| <= e_3 / m_2^(3/2) + (3/2) |skew| e_2 / m_2
        kurt  = m_4 / m_2^2 - 3:                       |d kurt| <= e_4 / m_2^2 + 2 (kurt + 3) e_2 / m_2.
    Each is doubled for the dropped terms of second order, and 2^-24 |value| is added for the one rounding of the image to
    float32."""
    n = Z.shape[0]
    a1, a2, a3, a4 = (z.sum(axis=0) / n for z in _powers(Z))
    l1, l2, l3, l4 = (z.sum(axis=0) / n for z in _powers(np.abs(Z)))
    m2, m3, m4 = (z.mean(axis=0) for z in _powers(Z - a1[None, :])[1:])
    g = GAMMA
    e2 = g * (l2 + 2 * np.abs(a1) * l1)
    e3 = g * (l3 + 3 * np.abs(a1) * l2 + (3 * np.abs(a2) + 6 * a1 * a1) * l1)
    e4 = g * (l4 + 4 * np.abs(a1) * l3 + 6 * a1 * a1 * l2 + (4 * np.abs(a3) + 12 * np.abs(a1 * a2) + 12 * np.abs(a1) ** 3) * l1)
    std, skew, kurt = np.sqrt(m2), m3 / m2 ** 1.5, m4 / m2 ** 2 - 3.0
    ref = {"mean": a1, "std": std, "skewness": skew, "kurtosis": kurt}
    bound = {"mean": 2 * g * l1, "std": 2 * e2 / (2 * std), "skewness": 2 * (e3 / m2 ** 1.5 + 1.5 * np.abs(skew) * e2 / m2),
             "kurtosis": 2 * (e4 / m2 ** 2 + 2 * (kurt + 3.0) * e2 / m2)}
    floor_margin = (n * m2) / (3 * GAMMA * n * a2)         # > 1: the pixel is above the variance floor
    return ref, bound, floor_margin


def kinds64(pmd, mov):
    """{kind: ((T, D) float64 values, the (D,) centring vector the device uses)}: the movie, the float64 reconstruction
    and their difference, pixels in C order."""
    from localmd_amd import maps as MP

    T = mov.shape[0]
    X64 = den64(pmd, absolute=False).T
    Y64 = mov.reshape(T, -1).astype(np.float64)
    mean32 = np.asarray(pmd.mean_img, np.float32).reshape(-1).astype(np.float64)
    return {"raw": (Y64, MP.centring_vector(pmd).astype(np.float64)), "denoised": (X64, mean32),
            "residual": (Y64 - X64, np.zeros(Y64.shape[1]))}


def exported_kinds64(pmd, mov, panels):
    """kinds64 with the float32 values export_movie writes (``panels``) in the place of the float64 reconstruction and of
    its difference from the movie: the values the kernel sums, for which the bounds of moment_bounds are derived.  On a
    pixel whose denoised values vary by less than their own rounding to float32 (one weak column, no background) the
    distance of the expanded values from the float64 reconstruction - within den_bound, which check_export asserts - is
    more than moment_bounds allows for the sums, so the two steps are checked one after the other."""
    vals = kinds64(pmd, mov)
    return {k: (panels[k].astype(np.float64), vals[k][1]) for k in ALL}


def check_moments(s, pmd, mov, figures=None, vals=None):
    """mean / std / skewness / kurtosis of every kind against float64 NumPy: on the movie, on the float64 reconstruction
    and on their difference (``vals``: other values, as kinds64 returns them).  ``s``: an object with, or a dict of,
    {kind: {stat: image}}."""
    get = s.get if isinstance(s, dict) else (lambda k: getattr(s, k))
    d1, d2 = (int(x) for x in pmd.shape[1:])
    vals = kinds64(pmd, mov) if vals is None else vals
    for kind in ALL:
        Yk, centre = vals[kind]
        flat = np.ptp(Yk, axis=0) == 0
        if flat.any():
            # constant pixels (those no column of U touches: the denoised movie is the mean image there): the variance is
            # at the floor of summary.finish_moments and counts as zero; test_gpu_summary.
            # test_decomposition_without_columns_or_rank asserts the same of a whole constant movie
            assert kind == "denoised"
            assert np.array_equal(get(kind)["mean"].reshape(-1)[flat], Yk[0, flat].astype(np.float32))
            assert not any(get(kind)[stat].reshape(-1)[flat].any() for stat in ("std", "skewness", "kurtosis"))
            if flat.all():
                continue
        ref, bound, margin = moment_bounds(Yk[:, ~flat] - centre[None, ~flat])
        ref["mean"] = ref["mean"] + centre[~flat]
        print(kind, "variance / floor, smallest", margin.min())
        assert margin.min() > 1.0, kind                                  # no pixel at the floor: it hides nothing here
        for stat in MOMENTS:
            got = get(kind)[stat]
            assert got.shape == (d1, d2) and got.dtype == np.float32
            b = bound[stat] + U24 * np.abs(ref[stat])
            err = np.abs(got.reshape(-1)[~flat].astype(np.float64) - ref[stat])
            print(kind, stat, "max error / bound", (err / b).max(), "max error", err.max())
            if figures is not None:
                figures[kind + " " + stat] = float((err / b).max())
            assert np.all(err <= b), (kind, stat)


def check_pnr(s, pmd, mov, figures=None, vals=None):
    """pnr: (max - mean) / noise in float64 from the returned float32 max and the float64 mean, rounded once: 2^-23
    relative.  The raw sums of an integer movie about the dyadic centring vector are exact, so the float64 mean of NumPy
    is the one the host finished with; under the other kinds the device mean is within 2 GAMMA mean |z| of NumPy's
    (moment_bounds), which enters the ratio divided by the noise."""
    get = s.get if isinstance(s, dict) else (lambda k: getattr(s, k))
    d1, d2 = (int(x) for x in pmd.shape[1:])
    noise = np.asarray(pmd.var_img, np.float64).reshape(-1)
    assert np.all(np.isfinite(noise)) and np.all(noise > 0)
    for kind, (Yk, centre) in (kinds64(pmd, mov) if vals is None else vals).items():
        img = get(kind)
        assert img["pnr"].shape == (d1, d2) and img["pnr"].dtype == np.float32
        want = (img["max"].reshape(-1).astype(np.float64) - Yk.mean(axis=0)) / noise
        tol = 2.0 ** -23 * np.abs(want)
        if kind != "raw":
            tol = tol + 2 * GAMMA * np.abs(Yk - centre[None, :]).mean(axis=0) / noise
        err = np.abs(img["pnr"].reshape(-1) - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.nanmax(np.where(err > 0, err / tol, 0.0)))
        print(kind, "pnr: max error / tolerance", ratio)
        if figures is not None:
            figures[kind + " pnr"] = ratio
        assert np.all(err <= tol), kind


def run_summary(ctx, case, movie, fbs, resident=False):
    import localmd_amd
    from localmd_amd import summary as SM

    pmd = make_case(case)[0]
    s = localmd_amd.summary_images(pmd, movie, kinds=ALL, stats=SM.STATS, temporal_bin=case["summary_bin"],
                                   frame_batch_size=fbs, **({} if resident else {"ctx": ctx}))
    assert s.stats == SM.STATS and s.temporal_bin == case["summary_bin"]
    return {k: dict(getattr(s, k)) for k in ALL}


def check_summary(result, case, figures=None):
    """result: {kind: {stat: image}} and ``exported``, the float32 panels of export_movie."""
    pmd, X64, Y = make_case(case)
    assert np.array_equal(result["exported"]["raw"], Y.reshape(case["T"], -1))
    extrema_equal_export(result, result["exported"], case["d1"], case["d2"], case["summary_bin"])
    vals = exported_kinds64(pmd, Y, result["exported"])
    check_moments(result, pmd, Y, figures, vals)
    check_pnr(result, pmd, Y, figures, vals)


# ---- quantiles ------------------------------------------------------------------------------------------------------
def quantile_reference(S, q, interpolation):
    """(Q, D) float32 from the sorted (T, D) float32 values S, by the rules of the feature, written out here: h = q (T - 1)
    in float64; lower floor(h), higher ceil(h), nearest round-half-even(h); linear
    float32(lo + (hi - lo) (h - floor(h))) in float64."""
    n = S.shape[0]
    rows = []
    for x in q:
        h = np.float64(x) * (n - 1)
        lo, hi = int(np.floor(h)), int(np.ceil(h))
        if interpolation == "lower":
            rows.append(S[lo])
        elif interpolation == "higher":
            rows.append(S[hi])
        elif interpolation == "nearest":
            rows.append(S[int(np.rint(h))])
        else:
            lo64, hi64 = S[lo].astype(np.float64), S[hi].astype(np.float64)
            rows.append((lo64 + (hi64 - lo64) * (h - np.floor(h))).astype(np.float32))
    return np.stack(rows)


def mad_reference(panel, S):
    m = quantile_reference(S, (0.5,), "linear")[0]
    dev = np.abs(panel - m[None, :])                                  # one fp32 subtraction per element
    assert dev.dtype == np.float32
    return quantile_reference(np.sort(dev, axis=0), (0.5,), "linear")[0]


def quantiles_of(case):
    return (0.0, 0.5, 1.0, case["q"])


def run_quantiles(ctx, case, movie, fbs, resident=False):
    import localmd_amd

    pmd = make_case(case)[0]
    r = localmd_amd.quantile_images(pmd, movie, kinds=ALL, q=quantiles_of(case), mad=True, frame_batch_size=fbs,
                                    **({} if resident else {"ctx": ctx}))
    return {"q": _kinds(r), "mad": dict(r.mad)}


def check_quantiles(result, case, figures=None):
    """Exact against np.sort of the exported float32 movie (``exported`` in result)."""
    d1, d2, qs = case["d1"], case["d2"], quantiles_of(case)
    for kind in ALL:
        panel = result["exported"][kind]
        S = np.sort(panel, axis=0)
        got = result["q"][kind]
        assert got.shape == (len(qs), d1, d2) and got.dtype == np.float32
        assert got.tobytes() == quantile_reference(S, qs, "linear").tobytes(), kind
        mad = result["mad"][kind]
        assert mad.shape == (d1, d2) and mad.dtype == np.float32
        assert mad.tobytes() == mad_reference(panel, S).tobytes(), kind


# ---- rolling baseline -----------------------------------------------------------------------------------------------
def run_baseline(ctx, case, movie, fbs, resident=False):
    import localmd_amd

    pmd = make_case(case)[0]
    T, d1, d2 = case["T"], case["d1"], case["d2"]
    kw = dict(window=case["window"], temporal_bin=case["base_bin"], method=case["method"], frame_batch_size=fbs,
              q=case["base_q"] if case["method"] == "percentile" else None, **({} if resident else {"ctx": ctx}))
    out = {}
    for kind, mv in (("denoised", None), ("raw", movie)):
        bl = localmd_amd.rolling_baseline(pmd, mv, kind=kind, **kw)
        assert (bl.temporal_bin, bl.method, bl.kind, bl.n_frames) == (case["base_bin"], case["method"], kind, T)
        f = np.full((T, d1, d2), np.nan, np.float32)
        localmd_amd.dff_movie(pmd, f, mv, kind=kind, output=case["output"], **kw)
        out[kind] = {"knots": bl.knots, "frames": f}
    return out


def check_baseline(result, case, figures=None):
    """Bit for bit against baseline_ref / baseline_quantile_ref on the exported float32 movie (``exported`` in result)."""
    T, D, b = case["T"], case["d1"] * case["d2"], case["base_bin"]
    h = BR.half_of(case["window"], b)
    for kind in ("denoised", "raw"):
        y = result["exported"][kind]
        if case["method"] == "percentile":
            K, F = BQ.dff(y, b, h, case["base_q"], case["output"])
        else:
            K, F = BR.dff(y, b, h, case["method"], case["output"])
        knots = result[kind]["knots"]
        assert knots.shape == (-(-T // b), case["d1"], case["d2"]) and knots.dtype == np.float32
        assert knots.reshape(-1, D).tobytes() == K.tobytes(), (kind, "knots")
        assert result[kind]["frames"].reshape(T, D).tobytes() == F.tobytes(), (kind, case["output"])


# ---- projection -----------------------------------------------------------------------------------------------------
def run_project(ctx, case, movie, fbs, resident=False):
    pmd = make_case(case)[0]
    return {"C": pmd.project_frames(movie, frame_batch_size=fbs, **({} if resident else {"ctx": ctx}))}


def check_project(result, case, figures=None):
    """Against (U R)^T ((Y - mean) / std) in fp64 with the measure and the bound of
    test_gpu_projection.test_group_project_against_fp64: the error of every row, relative to the row of the same product
    of magnitudes (the scale of an fp32 fma chain's rounding), below 1e-6."""
    pmd, X64, Y = make_case(case)
    T = case["T"]
    mean, std, uc, rs, vt = factors64(pmd)
    ur = uc @ pmd.r.astype(np.float64)                                  # (D, rank), pixels in C order
    ys = (Y.reshape(T, -1).astype(np.float64) - mean[None, :]) / std[None, :]
    ref = ur.T @ ys.T
    scale = (np.abs(uc) @ np.abs(pmd.r.astype(np.float64))).T @ np.abs(ys).T
    C = result["C"]
    assert C.shape == (case["rank"], T) and C.dtype == np.float32 and np.all(np.isfinite(C))
    if not uc.shape[1]:
        assert not C.any()                                              # a U without columns projects onto nothing
        return
    err = np.linalg.norm(C - ref, axis=1) / np.linalg.norm(scale, axis=1)
    print("project_frames: max row err", err.max())
    if figures is not None:
        figures["row error / 1e-6"] = float(err.max() / 1e-6)
    assert err.max() < 1e-6, err.max()


# ---- superpixels ----------------------------------------------------------------------------------------------------
SP_KW = dict(th=1.0, cut_off=0.5, min_size=2)


def superpixels_equal_reference(sp, ref, cut_off, key):
    """``sp``: a Superpixels or a dict of its arrays."""
    get = sp.get if isinstance(sp, dict) else (lambda k: getattr(sp, k))
    nz = ref["rho"][ref["rho"] != 0]
    margin = np.abs(nz - cut_off).min() if nz.size else np.inf
    print(key, "K", len(ref["sizes"]), "of", ref["n_components"], "smallest |rho - cut_off|", margin)
    assert margin >= 1e-9, key                    # a property of the input: choose another seed if this ever fails
    assert get("threshold").dtype == np.float32 and get("threshold").tobytes() == ref["threshold"].tobytes(), key
    assert np.array_equal(get("edges"), ref["edges"]), key
    assert get("labels").dtype == np.int32 and np.array_equal(get("labels"), ref["labels"]), key
    assert get("sizes").dtype == np.int64 and np.array_equal(get("sizes"), ref["sizes"]), key
    assert get("n_components") == ref["n_components"], key
    assert get("correlation").dtype == np.float32 and np.abs(get("correlation") - ref["correlation"]).max() <= 1e-6, key


def run_superpixels(ctx, case, movie, fbs, resident=False):
    import localmd_amd

    pmd = make_case(case)[0]
    out = {}
    for kind, mv in (("denoised", None), ("raw", movie)):
        sp = localmd_amd.superpixels(pmd, mv, kind=kind, frame_batch_size=fbs, **SP_KW, **({} if resident else {"ctx": ctx}))
        out[kind] = {"labels": sp.labels, "sizes": sp.sizes, "correlation": sp.correlation, "threshold": sp.threshold,
                     "edges": sp.edges, "n_components": sp.n_components}
    return out


def check_superpixels(result, case, figures=None):
    from tests import superpixel_ref as SR

    T, d1, d2 = case["T"], case["d1"], case["d2"]
    for kind in ("denoised", "raw"):
        ref = SR.superpixels_ref(result["exported"][kind].reshape(T, d1, d2), **SP_KW)
        superpixels_equal_reference(result[kind], ref, SP_KW["cut_off"], (case["name"], kind))


# ---- demix ----------------------------------------------------------------------------------------------------------
def demix_rois(case):
    """The random discs of roi_masks and the planted ones, as far as no pixel is covered too often; the whole field last."""
    m = np.concatenate([roi_masks(case)[:4], planted(case)[0]])
    keep, seen = [], []
    for k in range(len(m)):
        if not any(np.array_equal(m[k], s) for s in seen):
            keep.append(k)
            seen.append(m[k])
    return np.concatenate([m[keep], np.ones((1,) + m.shape[1:], bool)])


def run_demix(ctx, case, movie=None, fbs=None, resident=False):
    import localmd_amd

    pmd = make_case(case)[0]
    dm = localmd_amd.demix(pmd, demix_rois(case), **({} if resident else {"ctx": ctx}))
    return {"traces": dm.traces, "footprints": dm.footprints.toarray(), "background": dm.background, "objective": dm.objective,
            "empty": dm.empty, "labels": np.asarray(dm.labels)}


_DEMIX_REF = {}


def demix_references(case):
    """(float64 reference, {output: the largest difference of the float32 emulation from it, relative to the largest
    reference value}): tests/hals_ref.demix_ref in both precisions on X64."""
    from tests import hals_ref as HR

    if case["name"] not in _DEMIX_REF:
        X64 = make_case(case)[1]
        rois = demix_rois(case)
        S = rois.reshape(len(rois), -1).T
        ref = HR.demix_ref(X64, S.astype(np.float64), S)
        r32 = HR.demix_ref(X64, S.astype(np.float64), S, dtype=np.float32)
        _DEMIX_REF[case["name"]] = (ref, {k: rel(r32[k], ref[k]) for k in ("traces", "footprints", "background", "objective")})
    return _DEMIX_REF[case["name"]]


# demix_ref with dtype=float32 (the emulations) against demix_ref in float64 on the one case of test_gpu_demix (24 x 20
# pixels, 300 frames, 5 ROIs), measured on the CPU: the largest difference relative to the largest reference value of each
# output.  The device is allowed 4 x that for the differing GEMM summation orders: traces 1.56e-6, footprints 7.49e-6,
# background 1.59e-7, objective 1.05e-6.
REF32 = {"traces": 3.90e-7, "footprints": 1.87e-6, "background": 3.97e-8, "objective": 2.61e-7}


def check_demix(result, case, figures=None):
    """As test_gpu_demix.test_demix_against_the_float64_reference: each output within 4 x the distance of the float32
    emulation (demix_ref with dtype=float32) from the float64 reference, the allowance for the differing GEMM summation
    orders.  That module holds the distances of its one case as constants (REF32).  They grow with the case (a trace of
    1100 frames over 9216 pixels is at 1.0e-6 where REF32 has 3.9e-7), so the distance is measured case by case; and as
    one measurement is one sample of the rounding noise, which on a field of 63 pixels can lie below the single rounding
    of a float32 output (background: 1.5e-9 against 2^-24 = 6e-8), the allowance is never below the one of that module:
    4 x max(REF32, the distance on this case)."""
    T, D = case["T"], case["d1"] * case["d2"]
    rois = demix_rois(case)
    K = len(rois)
    ref, ref32 = demix_references(case)
    ref32 = {k: max(v, REF32[k]) for k, v in ref32.items()}
    assert result["traces"].shape == (K, T) and result["traces"].dtype == np.float32
    assert result["footprints"].shape == (K, D) and result["footprints"].dtype == np.float32
    assert result["background"].shape == (case["d1"], case["d2"]) and result["background"].dtype == np.float32
    assert result["objective"].shape == (3,) and result["objective"].dtype == np.float64
    got = {"traces": result["traces"], "footprints": result["footprints"].T, "background": result["background"].reshape(-1),
           "objective": result["objective"]}
    for key, fp32 in ref32.items():
        r = rel(got[key], ref[key])
        print(key, "device vs float64:", r, "allowed:", 4 * fp32)
        if figures is not None:
            figures[key] = r / (4 * fp32) if fp32 else (0.0 if r == 0 else np.inf)
    for key, fp32 in ref32.items():
        assert rel(got[key], ref[key]) <= 4 * fp32, key
    assert np.all(np.diff(result["objective"]) <= 0)
    assert np.array_equal(result["empty"], ref["empty"])
    assert np.all(result["footprints"] >= 0) and np.array_equal(result["traces"].min(axis=1), np.zeros(K, np.float32))
    assert np.array_equal(result["footprints"] != 0, rois.reshape(K, -1) & (result["footprints"] != 0))


# ---- grow -----------------------------------------------------------------------------------------------------------
GROW_KW = dict(corr_th=0.3, halo=3, max_window=400)


def grown_equal_reference(g, ref, dm, d1, d2, corr_th, key):
    K = len(dm.labels)
    print(key, "status", ref["status"], "added", ref["added"], "removed", ref["removed"], "threshold", ref["threshold"],
          "smallest |rho - corr_th|", ref["margin"])
    assert ref["margin"] >= 1e-9, key                 # a property of the input: choose another seed if this ever fails
    assert list(g.status) == ref["status"], key
    assert np.array_equal(g.threshold, ref["threshold"]) and g.threshold.dtype == np.float64, key
    assert np.array_equal(g.added, ref["added"]) and np.array_equal(g.removed, ref["removed"]), key
    assert list(g.source) == sorted(ref["rows"]) and np.array_equal(g.labels, np.asarray(dm.labels)[g.source]), key
    assert g.rois.dtype == np.float32 and g.rois.shape == (len(g.source), d1 * d2) and g.rois.has_sorted_indices, key
    for row, k in enumerate(g.source):
        idx, val = ref["rows"][k]
        s, e = g.rois.indptr[row], g.rois.indptr[row + 1]
        assert np.array_equal(g.rois.indices[s:e], idx), (key, k)
        assert g.rois.data[s:e].tobytes() == val.tobytes(), (key, k)
    assert g.correlation.shape == (K, d1 * d2) and g.correlation.dtype == np.float32
    for k in range(K):
        s, e = g.correlation.indptr[k], g.correlation.indptr[k + 1]
        if k not in ref["rho"]:
            assert s == e, (key, k)
            continue
        i0, i1, j0, j1 = ref["win"][k]
        want_px = (np.arange(i0, i1)[:, None] * d2 + np.arange(j0, j1)[None, :]).reshape(-1)
        assert np.array_equal(g.correlation.indices[s:e], want_px), (key, k)
        assert g.correlation.data[s:e].tobytes() == ref["rho"][k].astype(np.float32).tobytes(), (key, k)


def grown_bytes(g):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (
        g.rois.data, g.rois.indices, g.rois.indptr, g.source, g.correlation.data, g.correlation.indices,
        g.correlation.indptr, g.threshold, g.added, g.removed)) + " ".join(g.status).encode()


def run_grow(ctx, case, movie, fbs, resident=False, demixed=None):
    """{"dm": the Demixed it grew from, kind: Grown}."""
    import localmd_amd

    pmd = make_case(case)[0]
    kw = {} if resident else {"ctx": ctx}
    dm = localmd_amd.demix(pmd, demix_rois(case), outer_iters=1, sweeps=2, **kw) if demixed is None else demixed
    return {"dm": dm, "denoised": localmd_amd.grow_rois(pmd, dm, frame_batch_size=fbs, **GROW_KW, **kw),
            "raw": localmd_amd.grow_rois(pmd, dm, movie, kind="raw", frame_batch_size=fbs, **GROW_KW, **kw)}


def check_grow(result, case, figures=None):
    from tests import grow_ref as GR

    T, d1, d2 = case["T"], case["d1"], case["d2"]
    dm = result["dm"]
    A = dm.footprints.toarray().astype(np.float32)
    for kind in ("denoised", "raw"):
        ref = GR.grow_ref(result["exported"][kind].reshape(T, d1, d2), A, dm.traces, d1, d2, **GROW_KW)
        grown_equal_reference(result[kind], ref, dm, d1, d2, GROW_KW["corr_th"], (case["name"], kind))


# ---- the bytes of a result --------------------------------------------------------------------------------------------
def bytes_of(x):
    """The bytes of every array of a result (dicts by sorted key), for the bitwise comparisons."""
    if isinstance(x, dict):
        return b"".join(k.encode() + bytes_of(x[k]) for k in sorted(x) if k not in ("exported", "getitem", "dm"))
    if isinstance(x, (list, tuple)):
        return b"".join(bytes_of(a) for a in x)
    if hasattr(x, "rois") and hasattr(x, "correlation"):
        return grown_bytes(x)
    return np.ascontiguousarray(x).tobytes() + str(np.asarray(x).dtype).encode()


RUN = {"export": run_export, "traces": run_traces, "maps": run_maps, "summary": run_summary, "quantiles": run_quantiles,
       "baseline": run_baseline, "project": run_project, "superpixels": run_superpixels, "demix": run_demix, "grow": run_grow}
CHECK = {"export": check_export, "traces": check_traces, "maps": check_maps, "summary": check_summary,
         "quantiles": check_quantiles, "baseline": check_baseline, "project": check_project,
         "superpixels": check_superpixels, "demix": check_demix, "grow": check_grow}
NEEDS_EXPORT = ("maps", "summary", "quantiles", "baseline", "superpixels", "grow")      # checked on the exported movie
USES_MOVIE = tuple(c for c in CONSUMERS if c != "demix")                                # demix reads the factors only
