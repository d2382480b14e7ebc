"""Host side of the ROI traces (localmd_amd.extract_traces, localmd_amd/traces.py): argument checks before any device
work, the tables of pmd_roi_gather for the three ROI forms (checked by a NumPy emulation of the kernel's sum), their
validation, and the sparse factor B = W diag(std) U of the denoised path.  No device needed: without one, Context(0)
raises, so a ValueError here shows the check ran first."""
import numpy as np
import pytest
import scipy.sparse

import localmd_amd
from localmd_amd import _lib
from localmd_amd import traces as TR
from localmd_amd.dataset import lazy_data_loader
from localmd_amd.pmdarray import PMDArray
from tests.test_export_host import _random_tiled_u


def _pmd(T=300, d1=6, d2=7, rank=3, order="F"):
    rng = np.random.default_rng(0)
    D = d1 * d2
    u = scipy.sparse.random(D, 4, density=0.5, random_state=1, format="coo")
    return PMDArray(u, rng.standard_normal((4, rank)), np.ones(rank), rng.standard_normal((rank, T)), (T, d1, d2), order,
                    rng.standard_normal((d1, d2)), np.ones((d1, d2)))


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a device context fails the test: the checks must come first."""
    def refuse(*a, **k):
        raise AssertionError("a device context was opened before the argument checks")
    monkeypatch.setattr(_lib.Context, "__init__", refuse)


class _Untouchable(lazy_data_loader):
    """A movie of the right shape whose frames must never be read."""

    def __init__(self, shape):
        self._shape = shape

    dtype = property(lambda self: np.float32)
    shape = property(lambda self: self._shape)

    def _compute_at_indices(self, indices):
        raise AssertionError("the movie was read")


def test_reexported():
    assert localmd_amd.extract_traces is TR.extract_traces
    assert "extract_traces" in localmd_amd.__all__
    assert callable(PMDArray.traces)


# ---- argument errors -----------------------------------------------------------------------------------------------
def _bad_calls():
    mov = _Untouchable((300, 6, 7))
    ok = np.zeros((2, 6, 7), bool)
    ok[0, 1:3, 2:4] = True
    ok[1, 4, 5] = True
    empty_roi = ok.copy()
    empty_roi[1] = False
    w = ok.astype(np.float64)
    nan_w, inf_w, zero_sum, neg_sum = w.copy(), w.copy(), w.copy(), w.copy()
    nan_w[0, 1, 2] = np.nan
    inf_w[0, 1, 2] = np.inf
    zero_sum[0, 1, 2:4] = (1.0, -1.0)
    zero_sum[0, 2, 2:4] = (2.0, -2.0)
    neg_sum[1, 4, 5] = -3.0
    labels_f = np.zeros((6, 7), np.float32)
    labels_f[2, 2] = 1.0
    labels_neg = np.zeros((6, 7), np.int32)
    labels_neg[2, 2] = -1
    return [
        dict(rois=ok, kinds="noise"),
        dict(rois=ok, kinds=()),
        dict(rois=ok, kinds=("raw", "raw"), movie=mov),
        dict(rois=ok, kinds=("denoised", "denoised")),
        dict(rois=ok, kinds=3),
        dict(rois=ok, reduce="median"),
        dict(rois=ok, kinds=("raw",)),                                           # raw without a movie
        dict(rois=ok, kinds=("denoised", "residual")),                           # residual without a movie
        dict(rois=ok, kinds="raw", movie=_Untouchable((300, 6, 8))),
        dict(rois=ok, kinds="raw", movie=np.zeros((299, 6, 7), np.float32)),
        dict(rois=ok, kinds="denoised", movie=np.zeros((299, 6, 7), np.float32)),
        dict(rois=np.zeros((2, 6, 8), bool)),                                    # wrong field of view
        dict(rois=np.ones((2, 7, 6), bool)),
        dict(rois=np.ones((2, 2, 6, 7), bool)),
        dict(rois=np.ones(42, bool)),
        dict(rois=np.ones((6, 8), np.int32)),                                    # label image of the wrong shape
        dict(rois=labels_f),                                                     # label image that is not integer
        dict(rois=np.ones((6, 7), bool)),
        dict(rois=labels_neg),
        dict(rois=np.zeros((6, 7), np.int32)),                                   # no label: K = 0
        dict(rois=np.zeros((0, 6, 7), bool)),                                    # K = 0
        dict(rois=scipy.sparse.csr_matrix((0, 42))),
        dict(rois=scipy.sparse.csr_matrix(np.ones((2, 41)))),                    # sparse with the wrong pixel count
        dict(rois=empty_roi),                                                    # an ROI without pixels
        dict(rois=scipy.sparse.csr_matrix(empty_roi.reshape(2, 42).astype(np.float64))),
        dict(rois=nan_w),
        dict(rois=inf_w, reduce="sum"),
        dict(rois=zero_sum, reduce="mean"),
        dict(rois=neg_sum, reduce="mean"),
        dict(rois=ok.astype(np.complex64)),
    ]


def test_argument_errors_before_any_device_work(no_device):
    pmd = _pmd()
    for kw in _bad_calls():
        kw = dict(kw)
        rois = kw.pop("rois")
        with pytest.raises(ValueError):
            localmd_amd.extract_traces(pmd, rois, **kw)
        with pytest.raises(ValueError):
            pmd.traces(rois, **kw)
    with pytest.raises(TypeError):
        localmd_amd.extract_traces(np.zeros((300, 6, 7)), np.ones((1, 6, 7), bool))


def test_no_frames_no_device(no_device):
    pmd = _pmd(T=0)
    tr = localmd_amd.extract_traces(pmd, np.ones((2, 6, 7), bool), np.zeros((0, 6, 7), np.uint16), kinds=("raw", "denoised"))
    assert tr.raw.shape == tr.denoised.shape == (2, 0) and tr.raw.dtype == np.float32 and tr.residual is None
    assert np.array_equal(tr.labels, [0, 1])


def test_sum_accepts_what_mean_refuses():
    """Weights that sum to zero or less are fine under reduce='sum' (tables only; no device)."""
    w = np.zeros((1, 6, 7))
    w[0, 1, 2:4] = (1.0, -1.0)
    t = TR.roi_tables(w, (6, 7), "F", "sum")
    assert t["K"] == 1 and np.array_equal(t["w"], np.array([1.0, -1.0], np.float32))
    with pytest.raises(ValueError):
        TR.roi_tables(w, (6, 7), "F", "mean")


# ---- tables --------------------------------------------------------------------------------------------------------
def _disc(d1, d2, ci, cj, r):
    ii, jj = np.mgrid[0:d1, 0:d2]
    return (ii - ci) ** 2 + (jj - cj) ** 2 <= r * r


def _roi_set(d1, d2, weighted, seed=0):
    """(K, d1, d2) float64 weights: two overlapping discs, a 1-pixel ROI, ROIs of 64 and 65 pixels, the whole field and
    a scattered ROI.  weighted: multiples of 1/4 in [1/4, 2] (exact in fp32 with an integer movie); else 0 / 1."""
    rng = np.random.default_rng(seed)
    masks = [_disc(d1, d2, 10, 12, 6.2), _disc(d1, d2, 13, 16, 5.1)]
    one = np.zeros((d1, d2), bool)
    one[d1 - 1, d2 - 1] = True
    masks.append(one)
    for npx in (64, 65):
        m = np.zeros(d1 * d2, bool)
        m[rng.choice(d1 * d2, npx, replace=False)] = True
        masks.append(m.reshape(d1, d2))
    masks.append(np.ones((d1, d2), bool))
    masks.append(rng.random((d1, d2)) < 0.3)
    assert (masks[0] & masks[1]).any()
    w = np.stack(masks).astype(np.float64)
    if weighted:
        w *= rng.integers(1, 9, w.shape) / 4.0
    return w


def _forms(w, order):
    """The same masks as a dense array and as a sparse matrix with columns in `order`."""
    K = w.shape[0]
    sp = scipy.sparse.csr_matrix(np.stack([w[k].reshape(-1, order=order) for k in range(K)]))
    return {"dense": w, "sparse": sp, "sparse_coo": sp.tocoo()}


def _emulate(t, Y):
    """pmd_roi_gather in fp32 NumPy for frames Y (n, D): per segment the 64 lane chains (lane l takes pixels l, l + 64,
    ...: a product and an addition per pixel; exact here, so fma or not is the same), the xor butterfly 1, 2, ..., 32,
    then the partial sums of a split ROI added in segment order from 0."""
    n = Y.shape[0]
    Yf = Y.astype(np.float32)
    out = np.full((t["K"], n), np.nan, np.float32)
    ws = np.full((max(t["n_partial_rows"], 1), n), np.nan, np.float32)
    lane_id = np.arange(64)
    for q0, p, out_row, to_ws in t["segs"]:
        lanes = np.zeros((64, n), np.float32)
        for q in range(0, p, 64):
            m = min(64, p - q)
            idx = np.arange(q0 + q, q0 + q + m)
            lanes[:m] = t["w"][idx][:, None] * Yf[:, t["pix"][idx]].T + lanes[:m]
        for step in (1, 2, 4, 8, 16, 32):
            lanes = lanes + lanes[lane_id ^ step]
        assert np.all(lanes == lanes[0])                      # every lane ends with the same bits
        (ws if to_ws else out)[out_row] = lanes[0]
    for out_row, row0, parts in t["split"]:
        s = np.zeros(n, np.float32)
        for c in range(parts):
            s = s + ws[row0 + c]
        out[out_row] = s
    return out


@pytest.mark.parametrize("seg", [TR.ROI_SEG, 128])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("order", ["F", "C"])
def test_roi_tables_reproduce_the_weighted_sum_exactly(order, weighted, seg):
    d1, d2 = 36, 40
    D = d1 * d2
    assert D > TR.ROI_SEG                                     # the whole-field ROI is split
    w = _roi_set(d1, d2, weighted)
    W64 = w.reshape(w.shape[0], D)
    Y = np.random.default_rng(1).integers(0, 256, (5, D)).astype(np.float64)
    want = W64 @ Y.T
    assert np.abs(W64).sum(axis=1).max() * 255 * 4 < 2 ** 24  # every partial sum is exact in fp32
    first = None
    for name, rois in _forms(w, order).items():
        t = TR.roi_tables(rois, (d1, d2), order, "sum", seg=seg)
        TR.validate_roi_tables(t)
        assert t["K"] == w.shape[0] and np.array_equal(t["labels"], np.arange(w.shape[0]))
        assert np.all(t["segs"][:, 1] <= seg)
        npx = np.diff(t["ptr"])
        assert np.array_equal(npx, (W64 != 0).sum(axis=1))
        assert set(npx[[2, 3, 4, 5]]) == {1, 64, 65, D}
        n_split = int((npx > seg).sum())
        assert len(t["split"]) == n_split >= 1 and t["n_partial_rows"] == int((-(-npx // seg))[npx > seg].sum())
        for k in range(t["K"]):                               # ascending C-order ids: lanes read consecutive addresses
            assert np.all(np.diff(t["pix"][t["ptr"][k]:t["ptr"][k + 1]]) > 0)
        assert np.array_equal(t["W"].toarray(), W64)
        got = _emulate(t, Y)
        assert np.array_equal(got.astype(np.float64), want), name
        if first is None:
            first = t
        else:                                                 # the three forms describe the same masks: same tables
            for key in ("ptr", "pix", "w", "segs", "split"):
                assert np.array_equal(t[key], first[key]), (name, key)


def test_reduce_mean_divides_each_row_by_its_sum():
    d1, d2 = 36, 40
    w = _roi_set(d1, d2, True)
    W64 = w.reshape(w.shape[0], -1)
    t = TR.roi_tables(w, (d1, d2), "F", "mean")
    want = W64 / W64.sum(axis=1, keepdims=True)
    assert np.array_equal(t["W"].toarray(), want)
    assert np.array_equal(t["w"], want[want != 0].astype(np.float32))


@pytest.mark.parametrize("order", ["F", "C"])
def test_label_image_rows_in_ascending_label_order(order):
    d1, d2 = 36, 40
    lab = np.zeros((d1, d2), np.int32)
    lab[_disc(d1, d2, 20, 20, 5)] = 20
    lab[_disc(d1, d2, 8, 30, 4)] = 3
    lab[30:, :] = 7                                           # 240 pixels
    lab[0, 0] = 1000
    t = TR.roi_tables(lab, (d1, d2), order)
    assert np.array_equal(t["labels"], [3, 7, 20, 1000]) and t["labels"].dtype == np.int64
    masks = np.stack([lab == v for v in (3, 7, 20, 1000)])
    ref = TR.roi_tables(masks, (d1, d2), order)
    for key in ("ptr", "pix", "w", "segs", "split"):
        assert np.array_equal(t[key], ref[key]), key
    assert np.array_equal(t["W"].toarray(), masks.reshape(4, -1).astype(np.float64))
    t8 = TR.roi_tables(lab.astype(np.uint16), (d1, d2), order)
    assert np.array_equal(t8["pix"], t["pix"]) and np.array_equal(t8["labels"], t["labels"])


def test_validate_roi_tables_rejects_faults():
    d1, d2 = 36, 40
    good = TR.roi_tables(_roi_set(d1, d2, True), (d1, d2), "F", seg=128)
    TR.validate_roi_tables(good)
    D = d1 * d2
    last = len(good["segs"]) - 1
    for key, edit in [
        ("pix", lambda x: x.__setitem__(5, D)),                          # pixel outside the field
        ("pix", lambda x: x.__setitem__(0, -1)),
        ("pix", lambda x: x.__setitem__(slice(0, 2), x[1::-1].copy())),  # not ascending
        ("w", lambda x: x.__setitem__(3, np.nan)),
        ("ptr", lambda x: x.__setitem__(-1, x[-1] + 1)),                 # past the pixel list
        ("ptr", lambda x: x.__setitem__(1, 0)),                          # an ROI without pixels
        ("segs", lambda x: x.__setitem__((0, 1), x[0, 1] + 1)),          # overlaps the next segment
        ("segs", lambda x: x.__setitem__((last, 1), x[last, 1] + 1)),    # past the pixel list
        ("segs", lambda x: x.__setitem__((0, 1), 0)),
        ("segs", lambda x: x.__setitem__((0, 2), good["K"])),            # output row outside the result
        ("segs", lambda x: x.__setitem__((0, 2), 1)),                    # two segments write one row
        ("segs", lambda x: x.__setitem__((0, 3), 2)),
        ("segs", lambda x: x.__setitem__((0, 3), 1)),                    # a whole ROI sent to the workspace
        ("split", lambda x: x.__setitem__((0, 2), x[0, 2] + 1)),         # reads a workspace row nobody wrote
        ("split", lambda x: x.__setitem__((0, 1), 1)),
        ("split", lambda x: x.__setitem__((0, 0), 0)),                   # adds its parts into another ROI's row
        ("n_partial_rows", None),
    ]:
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        if edit is None:
            bad[key] = good[key] + 1
        else:
            edit(bad[key])
        with pytest.raises(ValueError):
            TR.validate_roi_tables(bad)


# ---- the denoised path's factors ------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["F", "C"])
def test_b_equals_the_dense_product(order):
    d1, d2, T, rank = 36, 40, 50, 5
    D = d1 * d2
    rng = np.random.default_rng(3)
    u = _random_tiled_u(d1, d2, 12, 10, order, 2, seed=7)
    n_cols = u.shape[1]
    pmd = PMDArray(u, rng.standard_normal((n_cols, rank)), np.linspace(5, 1, rank), rng.standard_normal((rank, T)),
                   (T, d1, d2), order, rng.uniform(100, 900, (d1, d2)), rng.uniform(0.5, 9, (d1, d2)))
    w = _roi_set(d1, d2, True)
    for reduce in ("sum", "mean"):
        W64 = w.reshape(w.shape[0], D)
        if reduce == "mean":
            W64 = W64 / W64.sum(axis=1, keepdims=True)
        u_of_c = np.arange(D).reshape((d1, d2), order=order).reshape(-1)        # C-order pixel -> row of U
        Uc = u.toarray().astype(np.float64)[u_of_c]
        want_B = (W64 * pmd.var_img.reshape(-1)[None, :]) @ Uc
        want_off = W64 @ pmd.mean_img.reshape(-1)
        for rois in _forms(w, order).values():
            t = TR.roi_tables(rois, (d1, d2), order, reduce)
            B, off = TR.denoised_factors(pmd, t["W"])
            assert scipy.sparse.issparse(B) and B.shape == (w.shape[0], n_cols) and B.dtype == np.float64
            np.testing.assert_allclose(B.toarray(), want_B, rtol=1e-12, atol=1e-12 * np.abs(want_B).max())
            np.testing.assert_allclose(off, want_off, rtol=1e-13)
            # a disc touches a few tiles only: B stays sparse
            assert B[0].nnz < n_cols / 2


def test_device_bytes_do_not_depend_on_the_length():
    a = TR.traces_device_bytes(128 * 128, 4096, 2, 200, 3, 0, 40000, 220, 1, 16, 9000, 50, 12, True, True, 3, False)
    b = TR.traces_device_bytes(128 * 128, 4096, 2, 200, 3, 0, 40000, 220, 1, 16, 9000, 50, 12, True, True, 10, False)
    assert a == b
    assert a >= 2 * 4096 * 128 * 128 * 2 + 2 * 3 * 200 * 4096 * 4
    with pytest.raises(ValueError):
        TR._check_fit(a, a - 1)
    TR._check_fit(a, a)
