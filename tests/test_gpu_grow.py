"""Growing ROI supports on the GPU (localmd_amd.grow, csrc/roigrow.hip): pmd_roi_window_moments_accumulate through the C
ABI against NumPy (exactly for integer data, bit for bit against the sequential chains of tests/grow_ref.py for float
data), its independence of the split into calls, of the leading dimensions, the element type, the pair's position and
its company, special values, bad arguments and a frame past 2^31 elements; grow_rois end to end against grow_ref on the
exported movie, its invariances, the number of reads of the movie and bounded device memory; refine_demix against demix
and against the composition of the three public calls, and the planted cells of test_gpu_superpixels.py."""
import ctypes
import importlib

import numpy as np
import pytest

import localmd_amd
from localmd_amd._lib import ptr
from localmd_amd._minitiff import write_tiff
from localmd_amd.dataset import TiffArray
from tests import bigbuf as B
from tests import grow_ref as GR
from tests.consumer_fuzz import grown_bytes as _bytes, grown_equal_reference as _check_against_reference
from tests.test_gpu_demix import _pmd, _rois, _same
from tests.test_gpu_large_offsets import big, put_input  # noqa: F401  (big: the module's own 8.6 GB buffer)
from tests.test_gpu_maps import _CountingU16, _long_pmd
from tests.test_gpu_superpixels import CELLS, _exported, _planted_cells, _raw_movie, _Untouchable
from tests.test_grow_host import _seeds
from tests.test_traces_host import _disc

pytestmark = pytest.mark.gpu
GX = importlib.import_module("localmd_amd.grow")
ERR_ARG = -2
_ELEM = {"float32": 0, "uint16": 1, "int16": 2}
NAME = "pmd_roi_window_moments_accumulate"


def _dev(ctx, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _padded(a, ld, fill):
    out = np.full((a.shape[0], ld), fill, dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out


def _tables(pairs):
    """The arrays of the kernel from [(pixel, ROI, [(other ROI, value), ...]), ...]."""
    oth = [o for _, _, os in pairs for o in os]
    return {"pair_px": np.array([p for p, _, _ in pairs], np.int32), "pair_k": np.array([k for _, k, _ in pairs], np.int32),
            "oth_ptr": np.concatenate([[0], np.cumsum([len(os) for _, _, os in pairs])]).astype(np.int64),
            "oth_k": np.array([l for l, _ in oth] or [0], np.int32), "oth_a": np.array([a for _, a in oth] or [0], np.float32)}


def _random_pairs(rng, n_pairs, D, K, counts, value):
    pairs = []
    for i in range(n_pairs):
        k = int(rng.integers(K))
        m = min(counts[i % len(counts)], K - 1)
        ls = np.sort(rng.choice([l for l in range(K) if l != k], m, replace=False)) if m else []
        pairs.append((int(rng.integers(D)), k, [(int(l), value(rng)) for l in ls]))
    return pairs


def _call(ctx, xd, src, ldx, D, n, ctd, ldct, K, pairs, start=None, f0=0):
    """One call on the n frames from row f0 of the device batch xd and of the traces ctd; returns mom."""
    t = _tables(pairs)
    mom = _dev(ctx, np.zeros((3, len(pairs))) if start is None else start)
    xat = ctypes.c_void_p(xd.data_ptr() + f0 * ldx * xd.element_size())
    cat = ctypes.c_void_p(ctd.data_ptr() + f0 * ldct * 4)
    td = {k: _dev(ctx, v) for k, v in t.items()}
    ctx.call(NAME, xat, _ELEM[src], ldx, D, n, cat, ldct, K, len(pairs), ptr(td["pair_px"]), ptr(td["pair_k"]),
             ptr(td["oth_ptr"]), ptr(td["oth_k"]), ptr(td["oth_a"]), ptr(mom))
    ctx.sync()
    return mom.cpu().numpy()


def _lists(pairs):
    return [p for p, _, _ in pairs], [k for _, k, _ in pairs], [os for _, _, os in pairs]


# ---- the kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pairs", (1, 63, 64, 65, 257, 1000))
def test_moments_exact_for_integer_data(gpu_ctx, n_pairs):
    """Integer movie, traces and footprint values: y = x - sum a c is an integer below 2^17 + 64 * 3 * 4, exact in fp32
    whatever the order, and every sum an integer below 2^53, so the chains equal NumPy's int64 sums exactly, for every
    length, number of ROIs and others, leading dimension and element type, with identical bits across the types."""
    D = 37
    rng = np.random.default_rng(n_pairs)
    for case, n in enumerate((1, 7, 8, 9, 1025)):
        K = (1, 5, 70)[(case + n_pairs) % 3]
        Ct = rng.integers(-4, 5, (n, K)).astype(np.float32)
        pairs = _random_pairs(rng, n_pairs, D, K, (0, 1, 2, 64), lambda r: float(r.integers(1, 4)))
        px, pk, others = _lists(pairs)
        assert K == 1 or max(len(o) for o in others) == min(64, K - 1) or n_pairs < 4
        W = np.zeros((n_pairs, K), np.int64)
        for i, os in enumerate(others):
            for l, a in os:
                W[i, l] += int(a)
        data = {"uint16": rng.integers(0, 65536, (n, D)).astype(np.uint16),
                "int16": rng.integers(-32768, 32768, (n, D)).astype(np.int16)}
        data["uint16"][0, :3], data["int16"][0, :3] = (65535, 32768, 40000), (-32768, -1, 32767)
        data["float32"] = data["int16"].astype(np.float32)
        got = {}
        for src, X in data.items():
            y = X.astype(np.int64)[:, px] - Ct.astype(np.int64) @ W.T
            c = Ct.astype(np.int64)[:, pk]
            want = np.stack([y.sum(axis=0), (y * y).sum(axis=0), (y * c).sum(axis=0)]).astype(np.float64)
            for ldx, ldct in ((D, K), (D + 3, K + 2)):
                fill = np.nan if src == "float32" else (9 if src == "uint16" else -9)
                xd, cd = _dev(gpu_ctx, _padded(X, ldx, fill)), _dev(gpu_ctx, _padded(Ct, ldct, np.nan))
                got[src, ldx] = _call(gpu_ctx, xd, src, ldx, D, n, cd, ldct, K, pairs)
                assert np.array_equal(got[src, ldx], want), (n_pairs, n, K, src, ldx)
        assert np.array_equal(_bits(got["float32", D]), _bits(got["int16", D + 3]))


@pytest.fixture(scope="module")
def float_case():
    """257 pairs on 41 pixels and 70 ROIs with 0, 1, 2 and 64 others, 1025 frames; the chains at 9, 1024 and 1025."""
    rng = np.random.default_rng(7)
    D, K, n = 41, 70, 1025
    X = (100.0 + 5.0 * rng.standard_normal((n, D))).astype(np.float32)
    Ct = rng.standard_normal((n, K)).astype(np.float32)
    pairs = _random_pairs(rng, 257, D, K, (0, 1, 2, 64), lambda r: float(np.float32(r.uniform(0.1, 2.0))))
    ref = {m: GR.pair_moments(X[:m], Ct[:m], *_lists(pairs)) for m in (9, 1024, 1025)}
    return X, Ct, pairs, ref


def test_moments_float_data_bit_for_bit_and_split_over_calls(gpu_ctx, float_case):
    X, Ct, pairs, ref = float_case
    n, D = X.shape
    K = Ct.shape[1]
    for ldx, ldct in ((D, K), (D + 5, K + 1)):
        xd, cd = _dev(gpu_ctx, _padded(X, ldx, np.nan)), _dev(gpu_ctx, _padded(Ct, ldct, np.nan))
        for m in (9, 1024, 1025):
            assert np.array_equal(_bits(_call(gpu_ctx, xd, "float32", ldx, D, m, cd, ldct, K, pairs)), _bits(ref[m])), (m, ldx)
        first = _call(gpu_ctx, xd, "float32", ldx, D, 1024, cd, ldct, K, pairs)
        both = _call(gpu_ctx, xd, "float32", ldx, D, 1, cd, ldct, K, pairs, start=first, f0=1024)
        assert np.array_equal(_bits(both), _bits(ref[1025])), ldx
        for cut in range(1, 9):
            first = _call(gpu_ctx, xd, "float32", ldx, D, cut, cd, ldct, K, pairs)
            both = _call(gpu_ctx, xd, "float32", ldx, D, 9 - cut, cd, ldct, K, pairs, start=first, f0=cut)
            assert np.array_equal(_bits(both), _bits(ref[9])), (cut, ldx)
    # the reference continues a stored state the same way
    part = GR.pair_moments(X[:4], Ct[:4], *_lists(pairs))
    assert np.array_equal(_bits(GR.pair_moments(X[4:9], Ct[4:9], *_lists(pairs), start=part)), _bits(ref[9]))


def test_moments_bits_do_not_depend_on_position_or_company(gpu_ctx, float_case):
    X, Ct, pairs, ref = float_case
    n, D = X.shape
    K = Ct.shape[1]
    xd, cd = _dev(gpu_ctx, X), _dev(gpu_ctx, Ct)
    want = ref[1025]
    heavy = [i for i, p in enumerate(pairs) if len(p[2]) == 64][0]
    for i in (0, heavy, 256):
        alone = _call(gpu_ctx, xd, "float32", D, D, n, cd, K, K, [pairs[i]])
        assert np.array_equal(_bits(alone[:, 0]), _bits(want[:, i])), i
        thrice = _call(gpu_ctx, xd, "float32", D, D, n, cd, K, K, [pairs[i]] * 3 + [pairs[1]] * 70 + [pairs[i]])
        for at in (0, 1, 2, 73):
            assert np.array_equal(_bits(thrice[:, at]), _bits(want[:, i])), (i, at)
    perm = np.random.default_rng(8).permutation(len(pairs))
    moved = _call(gpu_ctx, xd, "float32", D, D, n, cd, K, K, [pairs[i] for i in perm])
    assert np.array_equal(_bits(moved), _bits(want[:, perm]))


def test_moments_special_values(gpu_ctx, float_case):
    """A NaN or an infinity in X reaches the pairs of that pixel; one in Ct the pairs of that ROI and those that take it
    out as an other; every other pair keeps its bits."""
    X, Ct, pairs, ref = float_case
    n, D, K = 40, X.shape[1], Ct.shape[1]
    X, Ct = X[:n].copy(), Ct[:n].copy()
    X[3, 5], X[39, 7], X[0, 9] = np.nan, np.inf, -np.inf
    Ct[11, 2], Ct[39, 60] = np.nan, np.inf
    got = _call(gpu_ctx, _dev(gpu_ctx, X), "float32", D, D, n, _dev(gpu_ctx, Ct), K, K, pairs)
    want = GR.pair_moments(X, Ct, *_lists(pairs))
    hit = np.array([p in (5, 7, 9) or k in (2, 60) or any(l in (2, 60) for l, _ in os) for p, k, os in pairs])
    assert hit.any() and not hit.all()
    assert np.array_equal((~np.isfinite(got)).any(axis=0), hit)
    assert np.array_equal(got, want, equal_nan=True)
    clean = GR.pair_moments(float_case[0][:n], float_case[1][:n], *_lists(pairs))
    assert np.array_equal(_bits(got[:, ~hit]), _bits(clean[:, ~hit]))


def test_moments_no_pairs_and_bad_arguments_leave_mom_untouched(gpu_ctx):
    import torch

    lib, h = gpu_ctx.lib, gpu_ctx.handle
    D, K, n = 35, 3, 4
    x = torch.zeros((8, 40), dtype=torch.float32, device=gpu_ctx.device)
    ct = torch.ones((8, 4), dtype=torch.float32, device=gpu_ctx.device)
    t = {k: _dev(gpu_ctx, v) for k, v in _tables([(1, 0, [(1, 1.0)]), (2, 1, []), (3, 2, [(0, 2.0), (1, 3.0)])]).items()}
    mom = torch.full((3, 3), 7.0, dtype=torch.float64, device=gpu_ctx.device)
    names = ["X", "elem", "ldx", "D", "n", "Ct", "ldct", "K", "n_pairs", "pair_px", "pair_k", "oth_ptr", "oth_k", "oth_a", "mom"]
    good = [ptr(x), 0, 40, D, n, ptr(ct), 4, K, 3, ptr(t["pair_px"]), ptr(t["pair_k"]), ptr(t["oth_ptr"]), ptr(t["oth_k"]),
            ptr(t["oth_a"]), ptr(mom)]
    bad = [dict(n=0), dict(n=-1), dict(K=0), dict(D=0), dict(ldx=D - 1), dict(ldct=K - 1), dict(n_pairs=-1), dict(elem=3),
           dict(elem=-1), dict(X=None), dict(Ct=None), dict(pair_px=None), dict(pair_k=None), dict(oth_ptr=None),
           dict(oth_k=None), dict(oth_a=None), dict(mom=None), dict(n_pairs=(2 ** 31 - 1) * 256 + 1)]
    for kw in bad:
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        assert getattr(lib, NAME)(h, *a) == ERR_ARG, kw
        assert lib.pmd_last_error(h), kw
    assert b"too many pairs" in lib.pmd_last_error(h)
    # n_pairs == 0: success, nothing read or written, whatever the pointers
    a = list(good)
    a[names.index("n_pairs")] = 0
    assert getattr(lib, NAME)(h, *a) == 0
    for k in ("X", "Ct", "pair_px", "pair_k", "oth_ptr", "oth_k", "oth_a", "mom"):
        a[names.index(k)] = None
    assert getattr(lib, NAME)(h, *a) == 0
    gpu_ctx.sync()
    assert bool((mom == 7.0).all().item())
    assert getattr(lib, NAME)(h, *good) == 0
    gpu_ctx.sync()
    assert np.array_equal(mom.cpu().numpy()[0], [7.0 + n * (0 - 1.0), 7.0, 7.0 + n * (0 - 2.0 - 3.0)])


@pytest.mark.parametrize("src", list(_ELEM))
def test_moments_movie_stride_past_2_31(gpu_ctx, big, src):  # noqa: F811
    """Three frames of 12 x 12 pixels at ldx = 2^30 + 4099: frame 2 starts at element 2^31 + 8198.  Small integers, exact;
    the places a 32-bit offset would reach hold the poison."""
    tag = {"float32": "f32", "uint16": "u16", "int16": "i16"}[src]
    geo = B.GEOMETRIES[f"frames_{tag}"]
    D, n, K = geo.live, 3, 3
    rng = np.random.default_rng(31)
    X = rng.integers(0 if src == "uint16" else -30, 31, (n, D)).astype(src)
    v = put_input(gpu_ctx, big, src, geo, X)
    Ct = rng.integers(-4, 5, (n, K)).astype(np.float32)
    pairs = _random_pairs(rng, 200, D, K, (0, 1, 2), lambda r: float(r.integers(1, 4)))
    px, pk, others = _lists(pairs)
    got = _call(gpu_ctx, v, src, B.STRIDE, D, n, _dev(gpu_ctx, Ct), K, K, pairs)
    y = X.astype(np.int64)[:, px] - np.stack([sum((int(a) * Ct[:, l].astype(np.int64) for l, a in os), np.zeros(n, np.int64))
                                              for os in others], axis=1)
    c = Ct.astype(np.int64)[:, pk]
    assert np.array_equal(got, np.stack([y.sum(axis=0), (y * y).sum(axis=0), (y * c).sum(axis=0)]).astype(np.float64))


# ---- grow_rois ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e(gpu_ctx):
    pmd = _pmd("F")
    X = _exported(gpu_ctx, pmd)
    return pmd, X, _raw_movie(X), pmd.demix(_rois(), ctx=gpu_ctx)


@pytest.mark.parametrize("kind", ["denoised", "raw"])
def test_grow_rois_equal_the_reference_on_the_exported_movie(gpu_ctx, e2e, kind):
    """Four discs, two of them overlapping, under a full-field ROI whose window (480 pixels) is above max_window: it stays
    fixed and is taken out of every pixel of the others."""
    pmd, X, raw, dm = e2e
    T, d1, d2 = pmd.shape
    movie = {"denoised": X, "raw": raw}[kind]
    A = dm.footprints.toarray().astype(np.float32)
    i0, i1, j0, j1 = GR.windows(A, d1, d2, 0)[4]
    assert (i1 - i0) * (j1 - j0) > 400 and (A[4] > 0).sum() > 200       # HALS has set some of its pixels to 0
    changed = 0
    for kw in (dict(corr_th=0.3, halo=3), dict(corr_th=0.1, halo=6, shrink=False), dict(corr_th=0.0, halo=2, max_size=30),
               dict(corr_th=0.3, halo=0, fixed=[1])):
        ref = GR.grow_ref(movie, A, dm.traces, d1, d2, max_window=400,
                          **dict(kw, fixed=np.isin(np.arange(5), kw.get("fixed", []))))
        g = localmd_amd.grow_rois(pmd, dm, raw if kind == "raw" else None, kind=kind, max_window=400, ctx=gpu_ctx, **kw)
        _check_against_reference(g, ref, dm, d1, d2, kw["corr_th"], (kind, kw))
        assert g.status[4] == "fixed" and ("fixed" not in kw or g.status[1] == "fixed")
        assert g.rois[4].toarray().tobytes() == A[4:5].tobytes()
        changed += int(g.added.sum() + g.removed.sum())
    assert changed > 0
    # the full-field ROI is subtracted as an other: without it (an empty ROI) the correlations are others
    g = localmd_amd.grow_rois(pmd, dm, raw if kind == "raw" else None, kind=kind, corr_th=0.3, halo=3, max_window=400, ctx=gpu_ctx)
    bare = localmd_amd.Demixed(dm.traces, dm.footprints.multiply((np.arange(5) != 4)[:, None].astype(np.float32)).tocsr(),
                               dm.background, dm.labels, dm.objective, dm.empty)
    g0 = pmd.grow_rois(bare, raw if kind == "raw" else None, kind=kind, corr_th=0.3, halo=3, max_window=400, ctx=gpu_ctx)
    assert g0.status[4] == "empty" and list(g0.source) == [0, 1, 2, 3]
    assert np.array_equal(g0.correlation.indices, g.correlation.indices)
    assert g0.correlation.data.tobytes() != g.correlation.data.tobytes()


def test_invariance_over_batches_sources_residency_and_order(gpu_ctx, tmp_path):
    import torch

    n = 2500
    pmd = _pmd("F", T=n)
    raw = _raw_movie(_exported(gpu_ctx, pmd))
    assert raw.min() >= 0 and raw.max() < 65535
    dm = pmd.demix(_rois(), outer_iters=1, sweeps=2, ctx=gpu_ctx)
    kw = dict(corr_th=0.2, halo=4, max_window=400, ctx=gpu_ctx)
    den = localmd_amd.grow_rois(pmd, dm, **kw)
    ref = localmd_amd.grow_rois(pmd, dm, raw, kind="raw", **kw)
    want_d, want_r = _bytes(den), _bytes(ref)
    assert want_d != want_r and den.correlation.nnz > 0
    for fbs in (64, 1000):
        assert _bytes(localmd_amd.grow_rois(pmd, dm, frame_batch_size=fbs, **kw)) == want_d, fbs
        assert _bytes(localmd_amd.grow_rois(pmd, dm, raw, kind="raw", frame_batch_size=fbs, **kw)) == want_r, fbs
    u16 = raw.astype(np.uint16)
    path = str(tmp_path / "movie.tif")
    write_tiff(path, u16)
    sources = {"uint16": u16, "tiff": TiffArray(path), "cpu_tensor": torch.from_numpy(raw),
               "device_tensor": torch.from_numpy(raw).to(gpu_ctx.device)}
    for name, src in sources.items():
        assert _bytes(localmd_amd.grow_rois(pmd, dm, src, kind="raw", frame_batch_size=1024, **kw)) == want_r, name
    pmd.to_device(ctx=gpu_ctx)
    try:
        assert _bytes(pmd.grow_rois(dm, corr_th=0.2, halo=4, max_window=400)) == want_d
        assert _bytes(pmd.grow_rois(dm, u16, kind="raw", corr_th=0.2, halo=4, max_window=400)) == want_r
    finally:
        pmd.to_host()
    pc = _pmd("C", T=n)                                       # the same movie decomposed in C order
    assert _bytes(localmd_amd.grow_rois(pc, dm, **kw)) == want_d
    assert _bytes(localmd_amd.grow_rois(pc, dm, raw, kind="raw", **kw)) == want_r


def _few_discs(d1, d2):
    return np.stack([_disc(d1, d2, 10, 12, 4.2), _disc(d1, d2, 13, 16, 4.2), _disc(d1, d2, 40, 30, 5.1)])


def test_reads_of_the_movie_and_bounded_memory(gpu_ctx):
    import torch

    d1 = d2 = 64
    n = 3000
    pmd = _long_pmd(n, d1, d2)
    dm = pmd.demix(_few_discs(d1, d2), outer_iters=1, sweeps=1, ctx=gpu_ctx)
    a = localmd_amd.grow_rois(pmd, dm, ctx=gpu_ctx)
    b = localmd_amd.grow_rois(pmd, dm, _Untouchable((n, d1, d2)), kind="denoised", ctx=gpu_ctx)      # never read
    assert _bytes(a) == _bytes(b)
    src = _CountingU16(n, d1, d2)
    localmd_amd.grow_rois(pmd, dm, src, kind="raw", frame_batch_size=1024, ctx=gpu_ctx)
    assert np.all(src.count == 1), np.unique(src.count)
    peaks, plan = {}, {}
    for m in (2048, 8192):
        pm = _long_pmd(m, d1, d2)
        dmm = pm.demix(_few_discs(d1, d2), outer_iters=1, sweeps=1, ctx=gpu_ctx)
        gpu_ctx.release_workspace()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        g = localmd_amd.grow_rois(pm, dmm, frame_batch_size=1024, ctx=gpu_ctx)
        peaks[m] = torch.cuda.max_memory_allocated() - base
    print("peak device bytes", peaks)
    assert peaks[8192] - peaks[2048] <= 1 << 20, peaks                      # the plan's slack
    tabs, xt = importlib.import_module("localmd_amd.export").expand_tables_for(pm)
    S = GX.supports(dmm.footprints)
    t = GX.pair_tables(dmm.footprints, GX.windows(S, d1, d2, 6), np.isin(g.status, ["grown", "lost", "oversize"]), d2)
    plan = GX.grow_device_bytes(D=d1 * d2, nb=1024, esize=4, kind="denoised", n_cols=pm.r.shape[0], rank=pm.r.shape[1],
                                n_entries=len(xt["entries"]), n_a=int(tabs["a"].size), n_patches=int(xt["n_patches"]),
                                host_source=True, n_batches=8, factors_on_device=False, K=3, n_pairs=len(t["pair_px"]),
                                n_others=len(t["oth_k"]))
    assert peaks[8192] <= plan, (peaks, plan)


# ---- refine_demix ---------------------------------------------------------------------------------------------------
def test_refine_demix_is_the_composition_of_the_three_calls(gpu_ctx):
    pmd, masks, traces = _planted_cells()
    T, d1, d2 = pmd.shape
    seeds = _seeds(d1, d2, CELLS)
    dm = pmd.demix(seeds, ctx=gpu_ctx)
    r0 = pmd.refine_demix(seeds, rounds=0, ctx=gpu_ctx)
    assert r0.rounds == [] and _same(r0.demixed, dm) and np.array_equal(r0.demixed.labels, dm.labels)
    gk, mk = dict(corr_th=0.8, halo=4), dict(corr_th=0.7)
    r = localmd_amd.refine_demix(pmd, seeds, rounds=2, grow_kw=gk, merge_kw=mk, ctx=gpu_ctx)
    assert len(r.rounds) == 2
    cur = dm
    for g_r, m_r in r.rounds:
        g = localmd_amd.grow_rois(pmd, cur, ctx=gpu_ctx, **gk)
        m = localmd_amd.merge_rois(g.rois, cur.traces[g.source], labels=g.labels, fixed=(g.status == "fixed")[g.source], **mk)
        assert _bytes(g) == _bytes(g_r)
        assert m.rois.toarray().tobytes() == m_r.rois.toarray().tobytes() and np.array_equal(m.labels, m_r.labels)
        assert [list(x) for x in m.groups] == [list(x) for x in m_r.groups]
        cur = pmd.demix(m.rois, ctx=gpu_ctx)
        cur.labels = m.labels                                 # what refine_demix carries over
    assert _same(r.demixed, cur) and np.array_equal(r.demixed.labels, m.labels)
    # the early stop: with every ROI fixed a round changes nothing, and the demix before it is the result
    r1 = pmd.refine_demix(seeds, rounds=3, grow_kw=dict(fixed=np.ones(5, bool)), ctx=gpu_ctx)
    assert len(r1.rounds) == 1 and list(r1.rounds[0][0].status) == ["fixed"] * 5 and _same(r1.demixed, dm)
    assert [list(x) for x in r1.rounds[0][1].groups] == [[k] for k in range(5)]
    r2 = pmd.refine_demix(seeds, rounds=1, merge=False, grow_kw=gk, ctx=gpu_ctx)
    assert r2.rounds[0][1] is None and _bytes(r2.rounds[0][0]) == _bytes(r.rounds[0][0])


def test_planted_cells_grow_back(gpu_ctx):
    """The assertions of tests/test_grow_host.py::test_planted_cells_grow_back_on_the_host (where the figures are) on the
    device: after one round from disc seeds of radius r - 1.3 the three isolated cells are recovered exactly, no support
    holds a pixel outside its cell, and 1 - corr of the traces of cells 3 and 4 with the planted ones falls at least 4x."""
    pmd, masks, traces = _planted_cells()
    T, d1, d2 = pmd.shape
    K, D = len(CELLS), d1 * d2
    M = masks.reshape(K, D)
    r = pmd.refine_demix(_seeds(d1, d2, CELLS), rounds=1, grow_kw=dict(corr_th=0.8, halo=4), ctx=gpu_ctx)
    g, m = r.rounds[0]
    before = pmd.demix(_seeds(d1, d2, CELLS), ctx=gpu_ctx)
    rho = g.correlation.data.astype(np.float64)
    print("status", g.status, "added", g.added, "smallest |rho - corr_th|", np.abs(rho[rho != 0] - 0.8).min())
    assert list(g.status) == ["grown"] * K and [list(x) for x in m.groups] == [[k] for k in range(K)]
    S1 = g.rois.toarray() > 0
    for k in (0, 1, 2):
        assert np.array_equal(S1[k], M[k]), k
    assert not (S1 & ~M).any()
    miss0 = [1.0 - float(np.corrcoef(before.traces[k], traces[k])[0, 1]) for k in range(K)]
    miss1 = [1.0 - float(np.corrcoef(r.demixed.traces[k], traces[k])[0, 1]) for k in range(K)]
    print("1 - corr before", miss0, "after one round", miss1)
    for k in (3, 4):
        assert miss1[k] * 4.0 <= miss0[k], (k, miss0[k], miss1[k])
