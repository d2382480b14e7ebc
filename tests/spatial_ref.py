"""Plain NumPy / SciPy statements of the separable spatial filter (localmd_amd.spatial, csrc/spatial.hip) and the planted
one-photon movies its tests use.

Conventions (binding): a frame is (d1, d2); a(y, x) = float(f[refl(y)][refl(x)]) with refl(i) = -1 - i below 0 and
2 d - 1 - i from d on (scipy.ndimage's mode="reflect", np.pad's mode="symmetric"); with weights wy (2 ry + 1), wx
(2 rx + 1), centre and box

    out[y][x] = centre a(y, x) + sum_{i, j} wy[i] wx[j] a(y + i - ry, x + j - rx) - box sum_{i, j} a(y + i - ry, x + j - rx).

The kernel's order: per source row the chain over the 2 rx + 1 taps ascending (products rounded, then added), then per
column the chain over the 2 ry + 1 rows ascending; the box sums likewise with plain adds; the centre product is added to
G and the box product subtracted last.  ``emulate`` is localmd_amd.spatial.filter_frames, which states that order in
NumPy float32.

The forward bound.  A term wy[i] wx[j] a of G passes through its product with wx (1 rounding), at most 2 rx adds of the
row chain, its product with wy (1), at most 2 ry adds of the column chain, the add of the centre term (1) and the final
subtraction (1): 2 rx + 2 ry + 4 roundings.  A term of the box sum passes through at most 2 rx + 2 ry adds, the product
with box (1) and the subtraction (1); the centre term through 3.  With n = 2 rx + 2 ry + 6 >= all of these, u = 2^-24 and
gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1 and 4.2):

    |computed - exact| <= gamma_n (|centre| |a| + sum |wy[i]| |wx[j]| |a| + box sum |a|)

for a float32 output without overflow (the weights are the fp32 ones on both sides; a 16-bit output adds its rounding).
"""
import numpy as np
from scipy import ndimage, signal

from localmd_amd.spatial import filter_frames as emulate  # noqa: F401  (the float32 statement of the contract)
from tests import register_ref as R

U = 2.0 ** -24


def refl(i, d):
    return -1 - i if i < 0 else (2 * d - 1 - i if i >= d else i)


def _sep64(a, wy, wx):
    h = ndimage.correlate1d(a, np.asarray(wx, dtype=np.float64), axis=-1, mode="reflect")
    return ndimage.correlate1d(h, np.asarray(wy, dtype=np.float64), axis=-2, mode="reflect")


def filter64(frames, filt):
    """The filter in float64 through scipy.ndimage.correlate1d(mode="reflect"); frames (..., d1, d2)."""
    a = np.asarray(frames, dtype=np.float64)
    out = _sep64(a, filt.wy, filt.wx)
    if filt.centre != 0:
        out = filt.centre * a + out
    if filt.box != 0:
        out = out - filt.box * _sep64(a, np.ones(2 * filt.ry + 1), np.ones(2 * filt.rx + 1))
    return out


def magnitude(frames, filt):
    """|centre| |a| + sum |wy| |wx| |a| + box sum |a|, float64."""
    a = np.abs(np.asarray(frames, dtype=np.float64))
    mag = abs(filt.centre) * a + _sep64(a, np.abs(filt.wy), np.abs(filt.wx))
    return mag + abs(filt.box) * _sep64(a, np.ones(2 * filt.ry + 1), np.ones(2 * filt.rx + 1))


def forward_bound(frames, filt):
    """The bound of |fp32 filter - exact filter| per pixel (module docstring), float64."""
    nu = (2 * filt.rx + 2 * filt.ry + 6) * U
    return nu / (1.0 - nu) * magnitude(frames, filt)


# ---- planted one-photon movies --------------------------------------------------------------------------------------
def hill(d1, d2, amplitude=3000.0, centre=(0.45, 0.55), width=(0.3, 0.3)):
    """A static Gaussian hill, fixed in the sensor frame: vignetting and out-of-focus fluorescence in one."""
    y, x = np.arange(d1)[:, None], np.arange(d2)[None, :]
    return amplitude * np.exp(-0.5 * (((y - centre[0] * d1) / (width[0] * d1)) ** 2
                                      + ((x - centre[1] * d2) / (width[1] * d2)) ** 2))


ONE_PHOTON = {
    "explicit": dict(T=24, d1=64, d2=96, max_shift=(4, 5), seed=7, noise=8.0),      # matched against the true base + hill
    "built": dict(T=40, d1=64, d2=96, max_shift=(2, 3), seed=11, noise=8.0),        # the template is built from the movie
}
SIGMA = 1.5
_cache = {}


def one_photon(name):
    """(movie (T, d1, d2) float32, template = base + hill (d1, d2) float32, planted shifts (T, 2)); cached, read-only."""
    if name not in _cache:
        c = ONE_PHOTON[name]
        mov, base, shifts = R.planted_movie(c["T"], c["d1"], c["d2"], c["max_shift"], seed=c["seed"], noise=c["noise"])
        hl = hill(c["d1"], c["d2"])
        out = ((mov.astype(np.float64) + hl).astype(np.float32), (base.astype(np.float64) + hl).astype(np.float32), shifts)
        for a in out:
            a.setflags(write=False)
        _cache[name] = out
    return _cache[name]


def match64(frames, template, max_shift):
    """Integer shifts (n, 2) and the float64 surfaces of ``frames`` against ``template`` (both as they are matched)."""
    tp = R.window_template(template, *max_shift)
    surf = np.stack([R.surface64(f, tp) for f in frames])
    return np.array([R.peak(s)[0] for s in surf], dtype=np.int64), surf


def peak_gap(surface):
    """(best - second best entry) of a surface, absolute."""
    v = np.sort(np.asarray(surface, dtype=np.float64).reshape(-1))
    return v[-1] - v[-2]


def propagated_bound(frame, template, filt, max_shift):
    """A bound on |surface of the fp32 pipeline - exact surface| for one raw frame and raw template: the correlation's own
    forward bound on the filtered inputs, plus the filter's forward bounds of the frame and of the template carried
    through the sum (|delta t'| <= bound_t + its window mean, since t' subtracts the window mean)."""
    my, mx = max_shift
    F, Tm = filter64(frame, filt), filter64(template, filt)
    tp = R.window_template(Tm.astype(np.float32), my, mx).astype(np.float64)
    own = R.forward_bound(F, tp, my, mx)
    bf, bt = forward_bound(frame, filt), forward_bound(template, filt)
    btw = bt[my:bt.shape[0] - my, mx:bt.shape[1] - mx]
    via_frame = signal.correlate2d(bf, np.abs(tp), mode="valid")
    via_template = signal.correlate2d(np.abs(F) + bf, btw + btw.mean(), mode="valid")
    return own + via_frame + via_template


def build_template64(movie, filt, max_shift, iters):
    """register_movie's built template in float64 on all frames of ``movie``: the mean, then ``iters`` times: match the
    filtered frames against the filtered current template, apply the integer shifts (nearest border) to the unfiltered
    frames, average.  ``filt`` None: no filter."""
    mov = np.asarray(movie, dtype=np.float64)
    seen = mov if filt is None else filter64(mov, filt)
    tmpl = mov.mean(axis=0)
    for _ in range(iters):
        cur = tmpl if filt is None else filter64(tmpl, filt)
        ints, _ = match64(seen, cur.astype(np.float32), max_shift)
        tmpl = np.stack([R.apply_frame(f, s, "nearest") for f, s in zip(mov, ints.astype(np.float64))]).mean(axis=0)
    return tmpl
