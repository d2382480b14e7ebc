"""
The diagnostic-image kernels and the two expansion primitives entry point by entry point (GPU): pmd_neighbour_moments,
pmd_lag_moments, pmd_neighbour_image, pmd_lag_image (csrc/diag.hip), pmd_diag_fused_accumulate (csrc/diag_fused.hip),
pmd_csr_rows_spmm and pmd_transpose_affine (csrc/expand.hip), called by name through the C ABI, each against the plain
NumPy reference of the same operation (tests/diag_ref.py), and make_pmd_diagnostic_images on hand-built decompositions.

Exact cases.  The movies are integer valued and every shifted value v a kernel forms (x - ref, w - w0, r - r0, and the
unshifted residual r of frame_ss) satisfies 64 v^2 < 2^24.  Every fp32 product, every fp32 sum of at most 64 of them, the
64-lane butterfly of frame_ss and every fp64 sum above them is then an integer below 2^24 resp. 2^53: exact, with or
without FMA contraction and in any summation order.  The device result must EQUAL the int64 reference; each test asserts
the precondition on its own inputs (_assert_exact_regime).  The spmm and transpose cases are exact in the same way.

Float cases, one per entry point, in the regime the kernels were written for (mean = 100 x std, not integer).  Per term:
at most two subtractions and a product, 3 u; a slice sum of 64 terms, 64 u; u = 2^-24.  So |got - want| <=
128 u sum|terms| elementwise, the sum of |terms| from the reference in float64; about twice the worst case.

Every output the contract says is overwritten is filled with NaN before the call, every workspace with 0xFF bytes;
output arrays have guard rows / columns that must keep their NaN; a refused call must leave its outputs as they were.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import diag_oracle as DO
from tests import diag_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ELEMS = {"f32": (0, np.float32, 0), "u16": (1, np.uint16, 40000), "i16": (2, np.int16, -1000)}   # code, dtype, offset
SHAPES = [(9, 31), (16, 16), (1, 300), (300, 1), (1, 1)]


def _t():
    import torch

    return torch


def P(t, byte_offset=0):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr() + int(byte_offset))


def _dev(ctx, a, dtype=None):
    return _t().from_numpy(np.array(a, dtype=dtype, order="C")).to(ctx.device)      # a copy: the cached cases are read-only


def _dev_bytes(ctx, a):
    """Any NumPy array as raw bytes on the device (the entry points take the element type as a code)."""
    return _t().from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(ctx.device)


def _nan(ctx, *shape, dtype="float64"):
    return _t().full(shape, float("nan"), dtype=getattr(_t(), dtype), device=ctx.device)


def _ws(ctx, nbytes):
    return _t().full((max(int(nbytes), 1),), 0xFF, dtype=_t().uint8, device=ctx.device)


def _host(ctx, t):
    ctx.sync()
    return t.cpu().numpy()


def _untouched(ctx, *tensors):
    ctx.sync()
    return all(bool(_t().isnan(t).all().item()) for t in tensors)


def _refused(ctx, match, name, *args):
    from localmd_amd._lib import PMDLibraryError

    with pytest.raises(PMDLibraryError, match=match):
        ctx.call(name, *args)


def _assert_exact_regime(*arrays):
    """64 v^2 < 2^24 for every value of every array: the precondition of the exact comparisons."""
    for a in arrays:
        assert a.dtype == np.int64
        m = int(np.abs(a).max())
        assert 64 * m * m < 2 ** 24, m


def _equal_int(got, want, msg=""):
    assert want.dtype == np.int64 and got.dtype == np.float64
    np.testing.assert_array_equal(got, want.astype(np.float64), err_msg=msg)


@functools.lru_cache(maxsize=None)
def _int_case(T, d1, d2):
    """mean in [900, 1100], y = mean + [-100, 100], w in [-60, 60]: |r| <= 160, every shifted value at most 320."""
    rng = np.random.default_rng(100003 * T + 1009 * d1 + d2)
    mean = rng.integers(900, 1101, (d1, d2))
    y = mean[None] + rng.integers(-100, 101, (T, d1, d2))
    w = rng.integers(-60, 61, (T, d1, d2))
    for a in (mean, y, w):
        a.setflags(write=False)
    return y, w, mean


@functools.lru_cache(maxsize=None)
def _float_case(T, d1, d2):
    """fp32 movie with mean = 100 x std (1000 and 10), a reconstruction with and without the mean, and the mean image."""
    rng = np.random.default_rng(7)
    mean = (1000.0 + 50.0 * rng.random((d1, d2))).astype(np.float32)
    signal = 3.0 * np.sin(2 * np.pi * np.arange(T) / 97.0)[:, None, None] * rng.standard_normal((1, d1, d2))
    w = signal.astype(np.float32)
    y = (mean[None] + signal + 10.0 * rng.standard_normal((T, d1, d2))).astype(np.float32)
    recon = (mean[None] + w).astype(np.float32)
    for a in (y, w, recon, mean):
        a.setflags(write=False)
    return y, w, recon, mean


# ---------------------------------------------------------------------------------- pmd_neighbour_moments
def _nm_call(ctx, a, b, ref, T, d1, d2, accumulate, mom, t0=0, ws_bytes=None):
    """pmd_neighbour_moments on the T frames of the device movies a (and b) from frame t0 on."""
    D = d1 * d2
    need = -(-T // 1024) * 10 * D * 8
    ws = _ws(ctx, need)
    ctx.call("pmd_neighbour_moments", P(a, 4 * t0 * D), P(b, 4 * t0 * D), P(ref), T, d1, d2, accumulate, P(mom), P(ws),
             need if ws_bytes is None else ws_bytes)


@functools.lru_cache(maxsize=None)
def _nm_reference(T, d1, d2, with_b):
    y, w, _ = _int_case(T, d1, d2)
    x = y - w if with_b else y
    _assert_exact_regime(x - x[0])
    mom, _ = R.neighbour_moments(y, w if with_b else None)
    return mom


NM_CASES = [(d1, d2, 130) for d1, d2 in SHAPES] + [(9, 31, T) for T in (1024, 1025, 2100)]


@pytest.mark.parametrize("with_b", [False, True], ids=["A", "A-B"])
@pytest.mark.parametrize("d1,d2,T", NM_CASES, ids=[f"{a}x{b}-T{T}" for a, b, T in NM_CASES])
def test_neighbour_moments_exact(gpu_ctx, d1, d2, T, with_b):
    """accumulate = 0 onto NaN: all ten rows, clamped neighbour slots included, equal the int64 reference.  D = 279 has a
    second pixel block of 23 live lanes, 16 x 16 fills one block exactly, single rows / columns / pixels clamp; T = 130
    ends on a slice of 2 frames, 1025 and 2100 on a ragged second / third frame block."""
    y, w, _ = _int_case(T, d1, d2)
    a, b = _dev(gpu_ctx, y, np.float32), (_dev(gpu_ctx, w, np.float32) if with_b else None)
    ref = _dev(gpu_ctx, (y - w if with_b else y)[0], np.float32)
    mom = _nan(gpu_ctx, 10, d1 * d2)
    _nm_call(gpu_ctx, a, b, ref, T, d1, d2, 0, mom)
    _equal_int(_host(gpu_ctx, mom), _nm_reference(T, d1, d2, with_b))


@pytest.mark.parametrize("with_b", [False, True], ids=["A", "A-B"])
def test_neighbour_moments_accumulate_chunks(gpu_ctx, with_b):
    """accumulate = 1 over chunks of 97, 1030 and 973 frames: the single call and the reference, bit for bit."""
    T, d1, d2 = 2100, 9, 31
    y, w, _ = _int_case(T, d1, d2)
    a, b = _dev(gpu_ctx, y, np.float32), (_dev(gpu_ctx, w, np.float32) if with_b else None)
    ref = _dev(gpu_ctx, (y - w if with_b else y)[0], np.float32)
    mom = _t().zeros((10, d1 * d2), dtype=_t().float64, device=gpu_ctx.device)
    for t0, t1 in ((0, 97), (97, 1127), (1127, T)):
        _nm_call(gpu_ctx, a, b, ref, t1 - t0, d1, d2, 1, mom, t0=t0)
    single = _nan(gpu_ctx, 10, d1 * d2)
    _nm_call(gpu_ctx, a, b, ref, T, d1, d2, 0, single)
    got = _host(gpu_ctx, mom)
    np.testing.assert_array_equal(got, _host(gpu_ctx, single))
    _equal_int(got, _nm_reference(T, d1, d2, with_b))


def test_neighbour_moments_workspace_one_byte_short(gpu_ctx):
    T, d1, d2 = 1025, 9, 31
    y, _, _ = _int_case(T, d1, d2)
    a, ref, mom = _dev(gpu_ctx, y, np.float32), _dev(gpu_ctx, y[0], np.float32), _nan(gpu_ctx, 10, d1 * d2)
    slices = 2
    assert gpu_ctx.lib.pmd_diag_workspace_bytes(T, d1 * d2) == slices * 10 * d1 * d2 * 8 + 4096
    from localmd_amd._lib import PMDLibraryError

    with pytest.raises(PMDLibraryError, match="workspace too small"):
        _nm_call(gpu_ctx, a, None, ref, T, d1, d2, 0, mom, ws_bytes=slices * 10 * d1 * d2 * 8 - 1)
    assert _untouched(gpu_ctx, mom)
    _nm_call(gpu_ctx, a, None, ref, T, d1, d2, 0, mom, ws_bytes=slices * 10 * d1 * d2 * 8)     # exactly enough
    _equal_int(_host(gpu_ctx, mom), _nm_reference(T, d1, d2, False))


def test_neighbour_moments_float(gpu_ctx):
    """x = movie - reconstruction (both with the mean: the subtraction is exact by Sterbenz), shifted by frame 0, in two
    accumulating calls; |got - want| <= 128 u sum|terms|."""
    T, d1, d2 = 700, 9, 31
    y, _, recon, _ = _float_case(T, d1, d2)
    for b_host in (None, recon):
        x0 = (y[0] - b_host[0]) if b_host is not None else y[0]
        assert x0.dtype == np.float32
        a, b, ref = _dev(gpu_ctx, y), (_dev(gpu_ctx, b_host) if b_host is not None else None), _dev(gpu_ctx, x0)
        mom = _nan(gpu_ctx, 10, d1 * d2)
        _nm_call(gpu_ctx, a, b, ref, 300, d1, d2, 0, mom)
        _nm_call(gpu_ctx, a, b, ref, T - 300, d1, d2, 1, mom, t0=300)
        want, _ = R.neighbour_moments(y, b_host, x0)
        bound = 128 * U * R.neighbour_moments(y, b_host, x0, absolute=True)[0]
        err = np.abs(_host(gpu_ctx, mom) - want)
        print("neighbour moments, B", b_host is not None, ": max err / bound", float((err / bound).max()))
        assert (err <= bound).all()


# ---------------------------------------------------------------------------------------- pmd_lag_moments
def _lag_call(ctx, a, ref, T, D, lag, accumulate, mom, t0=0, ws_bytes=None):
    need = max(-(-(T - lag) // 1024), 1) * 5 * D * 8
    ws = _ws(ctx, need)
    ctx.call("pmd_lag_moments", P(a, 4 * t0 * D), P(ref), T, D, lag, accumulate, P(mom), P(ws),
             need if ws_bytes is None else ws_bytes)


@functools.lru_cache(maxsize=None)
def _lag_reference(T, d1, d2, lag):
    y, _, _ = _int_case(T, d1, d2)
    _assert_exact_regime(y - y[0])
    return R.lag_moments(y, None, lag)


LAG_CASES = ([(d1, d2, 130, 3) for d1, d2 in SHAPES] + [(9, 31, 130, 129), (9, 31, 1024, 1), (9, 31, 1025, 1)] +
             [(9, 31, 2100, lag) for lag in (1, 3, 64, 1023, 1024, 1500)])


@pytest.mark.parametrize("d1,d2,T,lag", LAG_CASES, ids=[f"{a}x{b}-T{T}-lag{lag}" for a, b, T, lag in LAG_CASES])
def test_lag_moments_exact(gpu_ctx, d1, d2, T, lag):
    """accumulate = 0 onto NaN.  T - lag = 2099 ... 600 pairs: up to three frame blocks whose first frame is
    blockIdx.y * 1024 + lag; lag = T - 1 is the largest accepted lag (one pair)."""
    y, _, _ = _int_case(T, d1, d2)
    a, ref, mom = _dev(gpu_ctx, y, np.float32), _dev(gpu_ctx, y[0], np.float32), _nan(gpu_ctx, 5, d1 * d2)
    _lag_call(gpu_ctx, a, ref, T, d1 * d2, lag, 0, mom)
    _equal_int(_host(gpu_ctx, mom), _lag_reference(T, d1, d2, lag))


@pytest.mark.parametrize("lag", [3, 64])
def test_lag_moments_accumulate_chunks(gpu_ctx, lag):
    """Chunks of 97, 1030 and 973 new frames, each later chunk resident from `lag` frames before its first new frame."""
    T, d1, d2 = 2100, 9, 31
    D = d1 * d2
    y, _, _ = _int_case(T, d1, d2)
    a, ref = _dev(gpu_ctx, y, np.float32), _dev(gpu_ctx, y[0], np.float32)
    mom = _t().zeros((5, D), dtype=_t().float64, device=gpu_ctx.device)
    for t0, t1 in ((0, 97), (97, 1127), (1127, T)):
        lo = max(0, t0 - lag)
        _lag_call(gpu_ctx, a, ref, t1 - lo, D, lag, 1, mom, t0=lo)
    single = _nan(gpu_ctx, 5, D)
    _lag_call(gpu_ctx, a, ref, T, D, lag, 0, single)
    got = _host(gpu_ctx, mom)
    np.testing.assert_array_equal(got, _host(gpu_ctx, single))
    _equal_int(got, _lag_reference(T, d1, d2, lag))


def test_lag_moments_refusals(gpu_ctx):
    T, d1, d2 = 130, 9, 31
    D = d1 * d2
    y, _, _ = _int_case(T, d1, d2)
    a, ref, mom = _dev(gpu_ctx, y, np.float32), _dev(gpu_ctx, y[0], np.float32), _nan(gpu_ctx, 5, D)
    ws = _ws(gpu_ctx, 5 * D * 8)
    for lag in (T, 0):
        _refused(gpu_ctx, "lag", "pmd_lag_moments", P(a), P(ref), T, D, lag, 0, P(mom), P(ws), ws.numel())
    _refused(gpu_ctx, "workspace too small", "pmd_lag_moments", P(a), P(ref), T, D, 3, 0, P(mom), P(ws), 5 * D * 8 - 1)
    assert _untouched(gpu_ctx, mom)


def test_lag_moments_float(gpu_ctx):
    T, d1, d2, lag = 700, 9, 31, 3
    y, _, _, _ = _float_case(T, d1, d2)
    a, ref, mom = _dev(gpu_ctx, y), _dev(gpu_ctx, y[0]), _nan(gpu_ctx, 5, d1 * d2)
    _lag_call(gpu_ctx, a, ref, T, d1 * d2, lag, 0, mom)
    bound = 128 * U * R.lag_moments(y, None, lag, absolute=True)
    err = np.abs(_host(gpu_ctx, mom) - R.lag_moments(y, None, lag))
    print("lag moments: max err / bound", float((err / bound).max()))
    assert (err <= bound).all()


# ------------------------------------------------------------------------ pmd_neighbour_image / pmd_lag_image
IMG_T = 60
DEAD = {(9, 31): [(0, 0), (0, 5), (4, 10)], (1, 12): [(0, 4)], (12, 1): [(11, 0)], (1, 1): []}


@functools.lru_cache(maxsize=None)
def _image_moments(d1, d2):
    """fp64 moments of an integer movie, its stand-in reconstruction and their residual, shifted by the mean image, with
    zero-variance pixels in the movie at a corner, an edge and the interior; plus the lag-2 moments of the movie."""
    rng = np.random.default_rng(41 * d1 + d2)
    mean = rng.integers(900, 1101, (d1, d2))
    y = mean[None] + rng.integers(-100, 101, (IMG_T, d1, d2))
    w = rng.integers(-60, 61, (IMG_T, d1, d2)) + (y - mean[None]) // 2
    for i, j in DEAD[(d1, d2)]:
        y[:, i, j] = mean[i, j]
    my = R.neighbour_moments(y, None, mean)[0]
    mw = R.neighbour_moments(w, None, np.zeros_like(mean))[0]
    mr = R.neighbour_moments(y - mean[None], w, np.zeros_like(mean))[0]
    lag = R.lag_moments(y, mean, 2)
    # every centred sum of squares is at least a quarter of the raw one: cancellation costs at most a factor of 4
    for m in (my, mw, mr):
        assert (4 * (IMG_T * m[1] - m[0] * m[0]) >= IMG_T * m[1]).all()
    for s, ss in ((lag[0], lag[1]), (lag[2], lag[3])):
        assert (4 * ((IMG_T - 2) * ss - s * s) >= (IMG_T - 2) * ss).all()
    return tuple(m.astype(np.float64) for m in (my, mw, mr, lag)) + (y,)


def _same_image(got, want, msg):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=msg)
    np.testing.assert_array_equal(np.isinf(got), np.isinf(want), err_msg=msg)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, equal_nan=True, err_msg=msg)


@pytest.mark.parametrize("mode", [0, 1], ids=["max", "mean"])
@pytest.mark.parametrize("d1,d2", list(DEAD), ids=[f"{a}x{b}" for a, b in DEAD])
def test_neighbour_image(gpu_ctx, d1, d2, mode):
    """Both kinds against the float64 formulas at rtol 1e-12 (a dozen fp64 operations, cancellation at most 4: more than
    two orders above 12 * 4 * 2^-53), NaN and inf at the same pixels.  A zero-variance pixel gives 0 / 0 (kind 0) or
    x / 0 (kind 1) for its pairs: as the LAST existing neighbour it leaves NaN in the maximum, as an earlier one it is
    replaced by the next neighbour's value without the floor at 0."""
    D = d1 * d2
    my, mw, mr, _, y = _image_moments(d1, d2)
    dy, dw, dr = (_dev(gpu_ctx, m) for m in (my, mw, mr))
    out = _nan(gpu_ctx, D + 1)
    results = {}
    for name, num, hnum, kind in (("correlation", dy, my, 0), ("pmd", dw, mw, 1), ("residual", dr, mr, 1)):
        out.fill_(float("nan"))
        gpu_ctx.call("pmd_neighbour_image", P(num), P(dy) if kind else None, IMG_T, d1, d2, kind, mode, P(out))
        got = _host(gpu_ctx, out)
        assert np.isnan(got[D])                                         # the guard entry
        want = R.neighbour_image(hnum, my if kind else None, IMG_T, d1, d2, kind, mode)
        _same_image(got[:D], want, f"{name} mode {mode}")
        results[name] = got[:D].reshape(d1, d2)
    corr = results["correlation"]
    if (d1, d2) == (1, 1):
        assert np.isnan(corr[0, 0]) if mode == 1 else corr[0, 0] == 0.0     # no neighbour: 0 / 0, and the initial maximum
    if (d1, d2) == (9, 31):
        assert np.isnan(corr[3, 9])              # (4, 10) is its last neighbour
        assert np.isnan(corr[0, 0]) and np.isnan(corr[4, 10])
        if mode == 0:
            assert np.isfinite(corr[5, 11])      # (4, 10) is its first neighbour: replaced by the later ones
            later = [float(DO._corr(y[:, 5, 11], y[:, i, j])) for i, j in list(DO._neighbours(5, 11, 9, 31))[1:]]
            running = later[0]
            for v in later[1:]:
                running = max(v, running)
            np.testing.assert_allclose(corr[5, 11], running, rtol=1e-12)
        else:
            assert np.isnan(corr[5, 11])


@pytest.mark.parametrize("d1,d2", list(DEAD), ids=[f"{a}x{b}" for a, b in DEAD])
def test_lag_image(gpu_ctx, d1, d2):
    D = d1 * d2
    lag = _image_moments(d1, d2)[3]
    out, mom = _nan(gpu_ctx, D + 1), _dev(gpu_ctx, lag)
    gpu_ctx.call("pmd_lag_image", P(mom), D, IMG_T - 2, P(out))
    got = _host(gpu_ctx, out)
    assert np.isnan(got[D])
    want = R.lag_image(lag, IMG_T - 2)
    assert np.isnan(want).sum() == len(DEAD[(d1, d2)])
    _same_image(got[:D], want, "lag image")


def test_image_refusals(gpu_ctx):
    d1, d2 = 9, 31
    my, mw, _, lag, _ = _image_moments(d1, d2)
    dy, dw, dl, out = _dev(gpu_ctx, my), _dev(gpu_ctx, mw), _dev(gpu_ctx, lag), _nan(gpu_ctx, d1 * d2)
    for den, T, kind, mode in ((None, IMG_T, 1, 0), (dy, 1, 0, 0), (dy, IMG_T, 2, 0), (dy, IMG_T, 0, 2)):
        _refused(gpu_ctx, "pmd_neighbour_image", "pmd_neighbour_image", P(dw), P(den), T, d1, d2, kind, mode, P(out))
    _refused(gpu_ctx, "pmd_lag_image", "pmd_lag_image", P(dl), d1 * d2, 0, P(out))
    assert _untouched(gpu_ctx, out)


# ------------------------------------------------------------------------------- pmd_diag_fused_accumulate
class _Fused:
    """The inputs of one fused case on the host and the device, and its reference."""

    def __init__(self, ctx, T, d1, d2, elem, lag):
        self.ctx, self.T, self.d1, self.d2, self.D, self.lag = ctx, T, d1, d2, d1 * d2, lag
        self.code, self.dtype, offset = ELEMS[elem]
        y, w, mean = _int_case(T, d1, d2)
        y, mean = y + offset, mean + offset
        r = y - mean[None] - w
        _assert_exact_regime(y - y[0], w - w[0], r - r[0], r)
        self.y = y.astype(self.dtype).reshape(T, self.D)
        assert np.array_equal(self.y.astype(np.int64), y.reshape(T, self.D))       # the element type holds the values
        assert elem != "u16" or self.y.min() > 32767
        assert elem != "i16" or (self.y.min() < -100 and self.y.max() > 100)     # both signs
        self.want_mom, self.want_fss = R.fused_moments(y, w, mean, lag)
        self.want_ref = np.stack([y[0], w[0], r[0]]).reshape(3, self.D)
        self.W = _dev(ctx, w.reshape(T, self.D), np.float32)
        self.mean = _dev(ctx, mean.reshape(-1), np.float32)
        self.esize = self.y.dtype.itemsize

    def outputs(self):
        """moments zeroed (the call adds to them), ref and frame_ss full of NaN (the call overwrites them)."""
        mom = _t().zeros((35, self.D), dtype=_t().float64, device=self.ctx.device)
        return mom, _nan(self.ctx, 3, self.D, dtype="float32"), _nan(self.ctx, self.T + 1)

    def call(self, Y, ybase, ring, c0, n, out, lag=None, T=None, elem=None, ws_bytes=None):
        mom, ref, fss = out
        need = int(self.ctx.lib.pmd_diag_fused_workspace_bytes(n, self.D))
        assert need == -(-n // 512) * 35 * self.D * 8 + -(-self.D // 256) * n * 8
        ws = _ws(self.ctx, need)
        self.ctx.call("pmd_diag_fused_accumulate", P(Y), self.code if elem is None else elem, ybase, P(self.W, 4 * c0 * self.D),
                      P(ring), self.lag if lag is None else lag, c0, n, self.T if T is None else T, self.d1, self.d2, P(self.mean),
                      P(ref), P(mom), P(fss), P(ws), need if ws_bytes is None else ws_bytes)

    def resident(self, calls):
        """One resident movie, ybase = 0, no ring."""
        out = self.outputs()
        Y = _dev_bytes(self.ctx, self.y)
        for c0, n in calls:
            self.call(Y, 0, None, c0, n, out)
        return self.results(out)

    def batched(self, batches, block=512):
        """Every batch in a buffer of its own (ybase = the batch's first frame), cut into calls of `block` frames; after
        each batch the test writes the last `lag` frames read so far to ring slot (frame mod lag).  The ring has a guard
        row of 0xFF bytes after its `lag` slots, like everything of it that no batch has written yet."""
        out = self.outputs()
        lag = self.lag
        ring = np.full((lag + 1, self.D * self.esize), 0xFF, dtype=np.uint8)
        for b0, b1 in batches:
            Y = _dev_bytes(self.ctx, self.y[b0:b1])
            dring = _dev_bytes(self.ctx, ring) if b0 > 0 else None
            for c0 in range(b0, b1, block):
                self.call(Y, b0, dring, c0, min(block, b1 - c0), out)
            for t in range(max(b0, b1 - lag), b1):
                ring[t % lag] = self.y[t].view(np.uint8)
        return self.results(out)

    def results(self, out):
        mom, ref, fss = (_host(self.ctx, t) for t in out)
        assert np.isnan(fss[self.T])
        return mom, ref, fss[:self.T]

    def check(self, got, msg=""):
        mom, ref, fss = got
        _equal_int(mom, self.want_mom, msg + " moments")
        _equal_int(fss, self.want_fss, msg + " frame_ss")
        np.testing.assert_array_equal(ref, self.want_ref.astype(np.float32), err_msg=msg + " ref")


@pytest.mark.parametrize("lag", [1, 3, 64])
@pytest.mark.parametrize("elem", list(ELEMS))
def test_fused_one_call(gpu_ctx, elem, lag):
    """T = 130 in one call: 35 moments, frame_ss and ref equal the int64 reference; uint16 values above 32767 and int16
    values below 0 tell the two 16-bit types apart.  D = 279: the last pixel block has 23 live lanes in the butterfly."""
    case = _Fused(gpu_ctx, 130, 9, 31, elem, lag)
    case.check(case.resident([(0, 130)]))


FUSED_BATCHED = [(1, "f32"), (3, "f32"), (513, "f32"), (700, "f32"), (3, "u16"), (513, "i16")]


@pytest.mark.parametrize("lag,elem", FUSED_BATCHED, ids=[f"lag{lag}-{e}" for lag, e in FUSED_BATCHED])
def test_fused_batched(gpu_ctx, lag, elem):
    """T = 1100 as [0, 512), [512, 1024), [1024, 1100): a resident movie without ring, three batch buffers with ybase =
    c0 and a ring, and a single call of 1100 frames agree bit for bit with each other and with the reference.  lag 513
    crosses a whole 512-frame block; lag 700 is longer than a batch, so a batch rewrites only part of the ring and the
    third call reads slots written two calls earlier."""
    case = _Fused(gpu_ctx, 1100, 9, 31, elem, lag)
    calls = [(0, 512), (512, 512), (1024, 76)]
    a = case.resident(calls)
    b = case.batched([(c0, c0 + n) for c0, n in calls])
    c = case.resident([(0, 1100)])
    case.check(a, "resident")
    for other, name in ((b, "batched"), (c, "single call")):
        for x, y in zip(a, other):
            np.testing.assert_array_equal(x, y, err_msg=name)


@pytest.mark.parametrize("T,lag", [(1100, 3), (1100, 700), (1600, 3), (1600, 700)])
def test_fused_ybase_below_c0_with_ring(gpu_ctx, T, lag):
    """Batches [0, 1024) and [1024, T) in calls of 512 frames: the second call has ybase = 0 < c0 = 512; with T = 1600 the
    last call has ybase = 1024 < c0 = 1536 and, at lag 700, pairs that reach the ring."""
    case = _Fused(gpu_ctx, T, 9, 31, "f32", lag)
    case.check(case.batched([(0, 1024), (1024, T)]))


def test_fused_refusals(gpu_ctx):
    """Every refused call leaves moments and frame_ss as they were."""
    T, lag = 1100, 3
    case = _Fused(gpu_ctx, T, 9, 31, "f32", lag)
    Y = _dev_bytes(gpu_ctx, case.y)
    mom, ref, fss = _nan(gpu_ctx, 35, case.D), _nan(gpu_ctx, 3, case.D, dtype="float32"), _nan(gpu_ctx, T)
    out = (mom, ref, fss)
    ring = _ws(gpu_ctx, (lag + 1) * case.D * 4)
    from localmd_amd._lib import PMDLibraryError

    refusals = [("frames", dict(Y=Y, ybase=0, ring=None, c0=256, n=10)),
                ("frames", dict(Y=Y, ybase=0, ring=None, c0=1024, n=77)),
                ("frames", dict(Y=Y, ybase=1024, ring=ring, c0=512, n=10)),
                ("ybase", dict(Y=Y, ybase=1, ring=None, c0=0, n=10)),
                ("bad shape", dict(Y=Y, ybase=0, ring=None, c0=0, n=10, lag=T)),
                ("unknown element type", dict(Y=Y, ybase=0, ring=None, c0=0, n=10, elem=3)),
                ("ring", dict(Y=Y, ybase=512, ring=None, c0=512, n=10)),
                ("workspace too small", dict(Y=Y, ybase=0, ring=None, c0=0, n=10, ws_bytes=35 * case.D * 8 + 2 * 10 * 8 - 1))]
    for match, kw in refusals:
        with pytest.raises(PMDLibraryError, match=match):
            case.call(out=out, **kw)
    assert _untouched(gpu_ctx, mom, fss, ref)


def test_fused_float(gpu_ctx):
    """fp32 movie with mean = 100 x std in calls [0, 512) and [512, 700).  y - mean is exact (Sterbenz), so the residual
    costs one rounding, its shift another, the product a third: |got - want| <= 128 u sum|terms| with the shifts the
    call itself wrote to ref; those are y_0, w_0 exactly and r_0 to one rounding.  frame_ss: |r^2| to 3 u per pixel, six
    butterfly levels and four fp64 adds, inside 128 u sum r^2 as well."""
    T, d1, d2, lag = 700, 9, 31, 3
    D = d1 * d2
    y, w, _, mean = _float_case(T, d1, d2)
    Y, W, M = _dev(gpu_ctx, y), _dev(gpu_ctx, w), _dev(gpu_ctx, mean)
    mom = _t().zeros((35, D), dtype=_t().float64, device=gpu_ctx.device)
    ref, fss = _nan(gpu_ctx, 3, D, dtype="float32"), _nan(gpu_ctx, T)
    for c0, n in ((0, 512), (512, 188)):
        ws = _ws(gpu_ctx, gpu_ctx.lib.pmd_diag_fused_workspace_bytes(n, D))
        gpu_ctx.call("pmd_diag_fused_accumulate", P(Y), 0, 0, P(W, 4 * c0 * D), None, lag, c0, n, T, d1, d2, P(M), P(ref), P(mom),
                     P(fss), P(ws), ws.numel())
    got_ref = _host(gpu_ctx, ref).astype(np.float64)
    y64, w64, m64 = (v.astype(np.float64) for v in (y, w, mean))
    r0 = (y64[0] - m64 - w64[0]).reshape(-1)
    np.testing.assert_array_equal(got_ref[0], y64[0].reshape(-1))
    np.testing.assert_array_equal(got_ref[1], w64[0].reshape(-1))
    assert (np.abs(got_ref[2] - r0) <= 2 * U * (np.abs(y64[0] - m64).reshape(-1) + np.abs(w64[0]).reshape(-1))).all()
    want, want_fss = R.fused_moments(y, w, mean, lag, ref=got_ref)
    bound, bound_fss = R.fused_moments(y, w, mean, lag, ref=got_ref, absolute=True)
    err = np.abs(_host(gpu_ctx, mom) - want)
    err_fss = np.abs(_host(gpu_ctx, fss) - want_fss)
    print("fused moments: max err / bound", float((err / (128 * U * bound)).max()), "frame_ss",
          float((err_fss / (128 * U * want_fss)).max()))
    assert (err <= 128 * U * bound).all()
    assert (err_fss <= 128 * U * want_fss).all()


# -------------------------------------------------------------------------------------- pmd_csr_rows_spmm
SPMM_ROWS, SPMM_COLS, SPMM_LDMAX = 40, 23, 1040


@functools.lru_cache(maxsize=None)
def _spmm_case(integer):
    """40 x 23 CSR with rows of 0, 1, 7, 8, 9, 16, 17 and 23 nonzeros among others, a dense B of 23 x 1040, and a row
    selection of 57 entries with repeats.  integer: data and B in [-8, 8], sums below 23 * 64: exact in fp32."""
    rng = np.random.default_rng(19)
    lengths = np.array([0, 1, 7, 8, 9, 16, 17, 23] + list(rng.integers(0, 24, SPMM_ROWS - 8)))
    lengths = lengths[rng.permutation(SPMM_ROWS)]
    assert set([0, 1, 7, 8, 9, 16, 17, 23]) <= set(lengths.tolist())
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.permutation(SPMM_COLS)[:n]) for n in lengths]).astype(np.int32)
    if integer:
        data, B = rng.integers(-8, 9, indptr[-1]), rng.integers(-8, 9, (SPMM_COLS, SPMM_LDMAX))
        assert int(lengths.max()) * int(np.abs(data).max()) * int(np.abs(B).max()) < 2 ** 24       # every partial sum is exact
    else:
        data = rng.standard_normal(indptr[-1]).astype(np.float32)
        B = rng.standard_normal((SPMM_COLS, SPMM_LDMAX)).astype(np.float32)
    rows = np.concatenate([rng.permutation(SPMM_ROWS), rng.integers(0, SPMM_ROWS, 17)]).astype(np.int32)
    assert rows.size == 57
    return indptr, indices, data, B, rows


def _spmm_run(ctx, case, use_rows, ncols, ldb, ldo, out_offset=0):
    """out[:n_sel, :ncols] of the call; asserts that the columns [ncols, ldo), the guard row after the last row and the
    floats in front of an offset `out` keep their NaN."""
    indptr, indices, data, B, rows = case
    n_sel = rows.size if use_rows else SPMM_ROWS
    out = _nan(ctx, out_offset + (n_sel + 1) * ldo, dtype="float32")
    d_rows = _dev(ctx, rows) if use_rows else None
    d_indptr, d_indices, d_data = _dev(ctx, indptr), _dev(ctx, indices), _dev(ctx, data, np.float32)
    d_B = _dev(ctx, B[:, :ldb], np.float32)
    ctx.call("pmd_csr_rows_spmm", P(d_indptr), P(d_indices), P(d_data), P(d_rows), n_sel, P(d_B), ldb, ncols,
             P(out, 4 * out_offset), ldo)
    got = _host(ctx, out)
    assert np.isnan(got[:out_offset]).all()
    got = got[out_offset:].reshape(n_sel + 1, ldo)
    assert np.isnan(got[:n_sel, ncols:]).all() and np.isnan(got[n_sel]).all()
    return got[:n_sel, :ncols]


def _spmm_want(case, use_rows, ncols, **kw):
    indptr, indices, data, B, rows = case
    return R.csr_rows_spmm(indptr, indices, data, rows if use_rows else None, B, ncols, **kw)


@pytest.mark.parametrize("use_rows", [False, True], ids=["all-rows", "57-selected"])
@pytest.mark.parametrize("pad", [4, 5], ids=["ld-multiple-of-4", "ld-odd"])
@pytest.mark.parametrize("ncols", [1, 5, 255, 256, 260, 1028])
def test_spmm_exact(gpu_ctx, ncols, pad, use_rows):
    """ldb = ldo = (ncols rounded up to a multiple of 4) + pad.  pad 4 takes the float4 kernel from 256 columns on (a
    second blockIdx.y at 1028), pad 5 the scalar kernel at every width (a second blockIdx.y at 260 and 1028)."""
    case = _spmm_case(True)
    ld = (ncols + 3) // 4 * 4 + pad
    got = _spmm_run(gpu_ctx, case, use_rows, ncols, ld, ld)
    np.testing.assert_array_equal(got.astype(np.float64), _spmm_want(case, use_rows, ncols).astype(np.float64))


@pytest.mark.parametrize("ncols,ldb,ldo,offset", [(256, 259, 260, 0), (258, 260, 260, 0), (256, 260, 260, 1)],
                         ids=["ldb-259", "ncols-258", "out-plus-4-bytes"])
def test_spmm_gate_failures(gpu_ctx, ncols, ldb, ldo, offset):
    """One failed condition of the float4 gate each (ldb, ncols, the alignment of out): the scalar kernel gives the same
    exact result."""
    case = _spmm_case(True)
    got = _spmm_run(gpu_ctx, case, True, ncols, ldb, ldo, out_offset=offset)
    np.testing.assert_array_equal(got.astype(np.float64), _spmm_want(case, True, ncols).astype(np.float64))


def test_spmm_no_ops(gpu_ctx):
    indptr, indices, data, B, rows = _spmm_case(True)
    out = _nan(gpu_ctx, 57 * 8, dtype="float32")
    held = [_dev(gpu_ctx, indptr), _dev(gpu_ctx, indices), _dev(gpu_ctx, data, np.float32), _dev(gpu_ctx, rows)]
    args = [P(t) for t in held]
    dB = _dev(gpu_ctx, B[:, :8], np.float32)
    gpu_ctx.call("pmd_csr_rows_spmm", *args, 0, P(dB), 8, 8, P(out), 8)
    gpu_ctx.call("pmd_csr_rows_spmm", *args, 57, P(dB), 8, 0, P(out), 8)
    assert _untouched(gpu_ctx, out)


@pytest.mark.parametrize("ncols", [255, 1028])
def test_spmm_float(gpu_ctx, ncols):
    """General floats through both kernels: nnz products and nnz adds in any order, |got - want| <= (nnz + 1) u sum|terms|."""
    case = _spmm_case(False)
    ld = (ncols + 3) // 4 * 4 + 4
    got = _spmm_run(gpu_ctx, case, True, ncols, ld, ld).astype(np.float64)
    nnz = np.diff(case[0])[case[4]][:, None]
    bound = (nnz + 1) * U * _spmm_want(case, True, ncols, absolute=True)
    err = np.abs(got - _spmm_want(case, True, ncols))
    print("spmm: max err / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()


# ----------------------------------------------------------------------------------- pmd_transpose_affine
TA_SHAPES = [(1, 1), (31, 33), (32, 32), (70, 45), (300, 5)]


def _ta_run(ctx, src, scale, shift):
    """dst (cols, rows) of the call with lds_ = cols + 3 and ldd = rows + 5; the guard columns of dst and a guard row keep
    their NaN, the guard columns of src are NaN."""
    rows, cols = src.shape
    s = _nan(ctx, rows, cols + 3, dtype="float32")
    s[:, :cols] = _dev(ctx, src, np.float32)
    dst = _nan(ctx, cols + 1, rows + 5, dtype="float32")
    d_scale = None if scale is None else _dev(ctx, scale, np.float32)
    d_shift = None if shift is None else _dev(ctx, shift, np.float32)
    ctx.call("pmd_transpose_affine", P(s), cols + 3, rows, cols, P(d_scale), P(d_shift), P(dst), rows + 5)
    got = _host(ctx, dst)
    assert np.isnan(got[:cols, rows:]).all() and np.isnan(got[cols]).all()
    return got[:cols, :rows]


@pytest.mark.parametrize("with_shift", [False, True], ids=["no-shift", "shift"])
@pytest.mark.parametrize("with_scale", [False, True], ids=["no-scale", "scale"])
@pytest.mark.parametrize("rows,cols", TA_SHAPES, ids=[f"{r}x{c}" for r, c in TA_SHAPES])
def test_transpose_affine(gpu_ctx, rows, cols, with_scale, with_shift):
    """Integer src, power-of-two scale and integer shift: exact.  General floats: one rounding for the product and one
    for the sum (or one in all when they are fused), |got - want| <= u (|src scale| + |want|)."""
    rng = np.random.default_rng(rows * 100 + cols)
    src = rng.integers(-50, 51, (rows, cols))
    scale = 2 ** rng.integers(0, 4, rows) if with_scale else None
    shift = rng.integers(-300, 301, rows) if with_shift else None
    want = R.transpose_affine(src, scale, shift)
    assert want.dtype == np.int64 and np.abs(want).max() < 2 ** 24
    np.testing.assert_array_equal(_ta_run(gpu_ctx, src, scale, shift).astype(np.float64), want.astype(np.float64))

    fsrc = rng.standard_normal((rows, cols)).astype(np.float32)
    fscale = (8.0 * rng.random(rows) + 0.5).astype(np.float32) if with_scale else None
    fshift = (1000.0 * rng.standard_normal(rows)).astype(np.float32) if with_shift else None
    fwant = R.transpose_affine(fsrc, fscale, fshift)
    prod = R.transpose_affine(fsrc, fscale, None)
    err = np.abs(_ta_run(gpu_ctx, fsrc, fscale, fshift).astype(np.float64) - fwant)
    assert (err <= U * (np.abs(prod) + np.abs(fwant))).all()


# ------------------------------------------------------------------------------ make_pmd_diagnostic_images
DRV_T, DRV_D1, DRV_D2 = 2500, 8, 9


@functools.lru_cache(maxsize=None)
def _driver_case(order, dtype, offset):
    """A hand-built rank-3 PMDArray over an 8 x 9 field of view and 2500 frames (a small random sparse U, no decomposition
    is run), the integer movie mean + std * (U R s Vt) + noise it describes, and its dense expansion in float64.  The mean
    image holds multiples of 1/4, so movie - mean is exact in fp32."""
    import scipy.sparse
    from localmd_amd.pmdarray import PMDArray

    T, d1, d2 = DRV_T, DRV_D1, DRV_D2
    D = d1 * d2
    rng = np.random.default_rng(23)
    u = scipy.sparse.random(D, 5, density=0.3, random_state=4, format="csr", dtype=np.float32)
    r = rng.standard_normal((5, 3)).astype(np.float32)
    s = np.array([3.0, 2.0, 1.0], dtype=np.float32)
    v = (np.cumsum(rng.standard_normal((3, T)), axis=1) / 20.0).astype(np.float32)
    mean_img = (offset + np.rint(4 * (900.0 + 30.0 * rng.random((d1, d2)))) / 4).astype(np.float32)
    std_img = (6.0 + 4.0 * rng.random((d1, d2))).astype(np.float32)
    pmd = PMDArray(u, r, s, v, (T, d1, d2), order, mean_img, std_img)
    a = (u.astype(np.float64) @ (r.astype(np.float64) * s[None, :].astype(np.float64))) @ v.astype(np.float64)
    dense = mean_img.astype(np.float64)[None] + std_img.astype(np.float64)[None] * a[pmd.row_indices.reshape(-1)].T.reshape(T, d1, d2)
    movie = np.rint(dense + 8.0 * rng.standard_normal((T, d1, d2))).astype(dtype)
    return pmd, movie, dense


def _fp64_fields(movie, dense, mode, lag):
    y = movie.astype(np.float64)
    r = y - dense
    var_y = y.var(axis=0)
    assert (var_y > 0).all()
    return (DO.make_correlation_image(y, mode), DO.make_autocorrelation_image(y, lag), DO.make_pmd_correlation_image(y, dense, mode),
            DO.make_residual_correlation_image(y, dense, mode), r.std(axis=0), 1.0 - r.var(axis=0) / var_y,
            np.sqrt((r ** 2).mean(axis=(1, 2))))


@pytest.mark.parametrize("lag", [1023, 1024, 1500])
def test_driver_lag_at_and_beyond_the_batch(gpu_ctx, lag):
    """Batches of 1024 frames and a lag of a batch or more: each batch rewrites only part of the lag ring
    (_diagnostics.consume).  The autocorrelation against the oracle at the tolerances of test_gpu_diagnostics, and all
    seven fields bit-equal to the run that reads the movie as one batch (no ring at all)."""
    import localmd_amd

    pmd, movie, _ = _driver_case("C", np.float32, 0)
    got = localmd_amd.make_pmd_diagnostic_images(movie, pmd, lag=lag, frame_batch_size=1024, ctx=gpu_ctx)
    one = localmd_amd.make_pmd_diagnostic_images(movie, pmd, lag=lag, frame_batch_size=10 ** 6, ctx=gpu_ctx)
    np.testing.assert_allclose(got.autocorrelation, DO.make_autocorrelation_image(movie.astype(np.float64), lag), rtol=1e-5,
                               atol=1e-6)
    for name, x, y in zip(got._fields, got, one):
        np.testing.assert_array_equal(x, y, err_msg=name)


@pytest.mark.parametrize("mode", ["max", "mean"])
def test_driver_int16_source_with_negative_values(gpu_ctx, mode):
    import localmd_amd
    from tests.test_gpu_diagnostics import _check_close

    pmd, movie, dense = _driver_case("F", np.int16, -2000)
    assert movie.dtype == np.int16 and movie.max() < 0
    got = localmd_amd.make_pmd_diagnostic_images(movie, pmd, mode=mode, lag=2, frame_batch_size=1024, ctx=gpu_ctx)
    _check_close(got, _fp64_fields(movie, dense, mode, 2))


@pytest.mark.parametrize("variant", ["no_columns", "rank_zero"])
def test_driver_degenerate_decompositions(gpu_ctx, variant):
    """A decomposition without columns or of rank 0 reconstructs the mean image in every frame (the expand = False branch).
    pmd_correlation is what the formulas give for a constant reconstruction; the residual is movie - mean, whose cov
    (ddof 1) over var (ddof 0) is the correlation times T / (T - 1); movie - mean is exact in fp32 here, so the residual
    moments are the raw moments and the explained variance is exactly 0."""
    import localmd_amd
    from tests.util import degenerate_pmds

    pmd, movie, _ = _driver_case("C", np.float32, 0)
    T, d1, d2 = DRV_T, DRV_D1, DRV_D2
    flat = degenerate_pmds(pmd)[variant]
    y = movie.astype(np.int64)
    assert np.array_equal(y, movie) and y.var(axis=0).min() > 0
    den = R.neighbour_moments(y)[0]
    for mode, code in (("max", 0), ("mean", 1)):
        got = localmd_amd.make_pmd_diagnostic_images(movie, flat, mode=mode, lag=1, frame_batch_size=1024, ctx=gpu_ctx)
        want = R.neighbour_image(np.zeros((10, d1 * d2)), den, T, d1, d2, 1, code).reshape(d1, d2)
        np.testing.assert_array_equal(got.pmd_correlation, want)
        np.testing.assert_array_equal(want, 0.0)
        np.testing.assert_allclose(got.residual_correlation, got.correlation * (T / (T - 1.0)), rtol=1e-5, atol=0)
        np.testing.assert_array_equal(got.explained_variance, 0.0)
        np.testing.assert_allclose(got.correlation, DO.make_correlation_image(y.astype(np.float64), mode), rtol=1e-5, atol=1e-6)
