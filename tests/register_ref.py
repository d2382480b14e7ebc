"""Plain NumPy / SciPy statements of rigid registration by template matching (localmd_amd.register, csrc/register.hip).

Conventions (binding): a movie is (T, d1, d2); max_shift = (my, mx); the window is rows [my, d1 - my) x columns
[mx, d2 - mx) of the template, h x w >= 8 x 8; t' is the fp32 template on the window minus its window mean (float64,
rounded once); the surface of frame f is C[dy, dx] = sum over the window of t'[y, x] f[y + dy, x + dx], |dy| <= my,
|dx| <= mx = scipy.signal.correlate2d(f, t', mode="valid"); the shift maximises C (first maximum in row-major order, NaN
never wins, no finite entry: shift (0, 0) and peak NaN); the corrected frame is out[y, x] = f[y + dy, x + dx].

The kernel's summation order and its forward bound.  The window is cut into tiles of 32 rows x 64 columns.  Inside a
tile an accumulator is one fmaf chain (the product is not rounded) over at most L = min(32 / S, h) min(64, w) terms,
where S = 4, 2, 1 row ranges for (2 my + 1) ceil((2 mx + 1) / 8) <= 64, <= 128, above; the S ranges are added in
ascending order (S - 1 roundings), then the tiles in ascending order (tiles - 1 roundings).  A term therefore passes
through at most n = L + (S - 1) + (tiles - 1) roundings, and |computed - exact| <= gamma_n sum |t'| |f| with
gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).
"""
import numpy as np
from scipy import ndimage, signal

U = 2.0 ** -24


def window_template(template, my, mx):
    t = np.asarray(template, dtype=np.float32)
    win = t[my:t.shape[0] - my, mx:t.shape[1] - mx]
    return (win - np.float32(win.astype(np.float64).mean())).astype(np.float32)


def surface64(frame, tp):
    """The float64 surface (2 my + 1, 2 mx + 1) of one frame."""
    return signal.correlate2d(np.asarray(frame, dtype=np.float64), np.asarray(tp, dtype=np.float64), mode="valid")


def surface_brute(frame, tp, my, mx):
    f, t = np.asarray(frame, dtype=np.float64), np.asarray(tp, dtype=np.float64)
    h, w = t.shape
    out = np.zeros((2 * my + 1, 2 * mx + 1))
    for dy in range(-my, my + 1):
        for dx in range(-mx, mx + 1):
            s = 0.0
            for y in range(h):
                for x in range(w):
                    s += t[y, x] * f[my + y + dy, mx + x + dx]
            out[dy + my, dx + mx] = s
    return out


def roundings(d1, d2, my, mx):
    """n of the module docstring: the most roundings a term of the kernel's sum passes through."""
    h, w = d1 - 2 * my, d2 - 2 * mx
    items = (2 * my + 1) * -(-(2 * mx + 1) // 8)
    S = 4 if items <= 64 else (2 if items <= 128 else 1)
    tiles = -(-h // 32) * -(-w // 64)
    return min(32 // S, h) * min(64, w) + (S - 1) + (tiles - 1)


def forward_bound(frame, tp, my, mx):
    """The bound of |fp32 surface - exact surface| per entry, (2 my + 1, 2 mx + 1) float64."""
    d1, d2 = np.asarray(frame).shape
    mag = signal.correlate2d(np.abs(np.asarray(frame, dtype=np.float64)), np.abs(np.asarray(tp, dtype=np.float64)),
                             mode="valid")
    nu = roundings(d1, d2, my, mx) * U
    return nu / (1.0 - nu) * mag


def peak(surface):
    """((dy, dx), peak value, 3 x 3 neighbourhood with NaN outside the surface) under the tie and NaN rules."""
    s = np.asarray(surface)
    ny, nx = s.shape
    my, mx = ny // 2, nx // 2
    none = np.full((3, 3), np.nan, dtype=s.dtype)
    if not np.isfinite(s).any():
        return (0, 0), s.dtype.type(np.nan), none
    v = np.where(np.isnan(s), -np.inf, s)
    at = int(np.argmax(v))                       # the first maximum in row-major order
    py, px = divmod(at, nx)
    for a in range(3):
        for b in range(3):
            y, x = py + a - 1, px + b - 1
            if 0 <= y < ny and 0 <= x < nx:
                none[a, b] = s[y, x]
    return (py - my, px - mx), s[py, px], none


def subpixel_peak(neigh):
    """(oy, ox) float64 of one 3 x 3 neighbourhood: per axis (lo - hi) / (2 (lo - 2 c + hi)) clipped to [-0.5, 0.5];
    0 when one of lo, c, hi is not finite or the curvature lo - 2 c + hi is not negative."""
    nb = np.asarray(neigh, dtype=np.float64)
    out = []
    for lo, c, hi in ((nb[0, 1], nb[1, 1], nb[2, 1]), (nb[1, 0], nb[1, 1], nb[1, 2])):
        o = 0.0
        if np.isfinite(lo) and np.isfinite(c) and np.isfinite(hi):
            curv = lo - 2.0 * c + hi
            if curv < 0:
                o = float(np.clip(0.5 * (lo - hi) / curv, -0.5, 0.5))
        out.append(o)
    return np.array(out)


def quantize(v, dtype):
    dtype = np.dtype(dtype)
    v = np.asarray(v, dtype=np.float32)
    if dtype == np.float32:
        return v
    info = np.iinfo(dtype)
    with np.errstate(invalid="ignore"):
        q = np.clip(np.rint(v), info.min, info.max)
    return np.where(np.isnan(q), 0, q).astype(dtype)


def apply_frame(frame, shift, border="nearest", dtype=None):
    """One frame shifted: out[y, x] = f[y + dy, x + dx], operation by operation in fp32.  An integer shift copies (in the
    frame's own dtype unless ``dtype`` says otherwise); else with (iy, ix) = floor(shift), weights formed in float64 and
    rounded once, fl(fl(fl(w00 a) + fl(w01 b)) + fl(fl(w10 c) + fl(w11 d)))."""
    f = np.asarray(frame)
    d1, d2 = f.shape
    dy, dx = float(shift[0]), float(shift[1])
    iy, ix = int(np.floor(dy)), int(np.floor(dx))
    fy, fx = dy - iy, dx - ix
    w = [np.float32((1 - fy) * (1 - fx)), np.float32((1 - fy) * fx), np.float32(fy * (1 - fx)), np.float32(fy * fx)]
    whole = w[0] == 1 and w[1] == 0 and w[2] == 0 and w[3] == 0
    out_dtype = np.dtype(dtype) if dtype is not None else (f.dtype if whole else np.dtype(np.float32))
    constant = not isinstance(border, str)
    fill = np.float32(border) if constant else None
    ys, xs = np.arange(d1)[:, None], np.arange(d2)[None, :]

    def sample(oy, ox, as_float):
        y, x = ys + oy, xs + ox
        v = f[np.clip(y, 0, d1 - 1), np.clip(x, 0, d2 - 1)]
        if as_float:
            v = v.astype(np.float32)
        if constant:
            inside = (y >= 0) & (y < d1) & (x >= 0) & (x < d2)
            fv = fill if as_float else quantize(fill, out_dtype)
            v = np.where(inside, v, fv)
        return v

    if whole:
        if f.dtype == out_dtype:
            return sample(iy, ix, False).astype(out_dtype)
        return quantize(sample(iy, ix, True), out_dtype)
    a, b, c, d = sample(iy, ix, True), sample(iy, ix + 1, True), sample(iy + 1, ix, True), sample(iy + 1, ix + 1, True)
    with np.errstate(invalid="ignore", over="ignore"):
        top = np.float32(np.float32(w[0] * a) + np.float32(w[1] * b))
        bot = np.float32(np.float32(w[2] * c) + np.float32(w[3] * d))
        return quantize(np.float32(top + bot), out_dtype)


def apply_movie(movie, shifts, border="nearest", dtype=None):
    shifts = np.asarray(shifts, dtype=np.float64)
    whole = bool(np.all(shifts == np.floor(shifts)))
    if dtype is None:
        dtype = np.asarray(movie).dtype if whole else np.float32
    return np.stack([apply_frame(f, s, border, dtype) for f, s in zip(movie, shifts)])


def register_ref(movie, template, max_shift, subpixel=True, border="nearest", dtype=None, surfaces=None):
    """The whole function against an explicit template: dict of shifts (T, 2) float64, integer_shifts, peak, surfaces
    and the corrected movie.  ``surfaces`` given: the peaks are taken from them (the device's own), not recomputed."""
    my, mx = max_shift
    tp = window_template(template, my, mx)
    if surfaces is None:
        surfaces = np.stack([surface64(f, tp) for f in movie])
    ints, peaks, shifts = [], [], []
    for s in surfaces:
        (dy, dx), pk, nb = peak(s)
        off = subpixel_peak(nb) if subpixel else np.zeros(2)
        ints.append((dy, dx)), peaks.append(pk), shifts.append((dy + off[0], dx + off[1]))
    shifts = np.array(shifts, dtype=np.float64)
    return {"shifts": shifts, "integer_shifts": np.array(ints, dtype=np.int32), "peak": np.array(peaks),
            "surfaces": surfaces, "movie": apply_movie(movie, shifts, border, dtype)}


def same_bits(a, b):
    """Bit for bit, any NaN matching any NaN (the sign and payload of a produced NaN differ between processors)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and np.where(na, 0, a).tobytes() == np.where(nb, 0, b).tobytes()


def shift_bilinear(img, shift):
    """img sampled at (y + dy, x + dx) bilinearly in float64, edges clamped."""
    d1, d2 = img.shape
    y = np.arange(d1)[:, None] + shift[0]
    x = np.arange(d2)[None, :] + shift[1]
    y0, x0 = np.floor(y).astype(int), np.floor(x).astype(int)
    fy, fx = y - y0, x - x0
    g = lambda yy, xx: img[np.clip(yy, 0, d1 - 1), np.clip(xx, 0, d2 - 1)]   # noqa: E731
    return ((1 - fy) * (1 - fx) * g(y0, x0) + (1 - fy) * fx * g(y0, x0 + 1) + fy * (1 - fx) * g(y0 + 1, x0)
            + fy * fx * g(y0 + 1, x0 + 1))


def _smooth_path(rng, T, lo, hi, smooth):
    """T values that wander between lo and hi (both reached) on a time scale of ``smooth`` frames."""
    z = ndimage.gaussian_filter1d(rng.standard_normal(T + 6 * smooth), smooth)[3 * smooth:3 * smooth + T]
    return lo + (hi - lo) * (z - z.min()) / (z.max() - z.min())


def planted_movie(T, d1, d2, max_shift, seed, noise=8.0, fractional=False, n_blobs=None, dtype=np.float32, moving=True,
                  smooth=0):
    """(movie (T, d1, d2), base (d1, d2) float32, shifts (T, 2)): a Gaussian-blurred field of blobs on a larger canvas
    (about 100 .. 400 in value), cut at known offsets so that movie[t][y + dy_t, x + dx_t] ~ base[y, x]; every frame has
    its own gain in 0.8 .. 1.3 and additive Gaussian noise.  The first frame is unshifted and every extreme shift
    occurs.  ``smooth`` > 0: the (integer) shifts and the gains wander on that time scale instead of being drawn afresh
    for every frame, as tissue and lasers do (only then is motion something a decomposition keeps).  ``moving=False``:
    the same canvas, gains and noise with every shift 0.  ``fractional``: shifts uniform within one pixel of the limit
    (the nearest integer is never on the edge of the search range, where there is no parabola), the canvas sampled
    bilinearly."""
    my, mx = max_shift
    rng = np.random.default_rng(seed)
    M = max(my, mx) + 2
    H, W = d1 + 2 * M, d2 + 2 * M
    canvas = np.zeros((H, W))
    n_blobs = n_blobs or max(12, H * W // 60)
    canvas[rng.integers(0, H, n_blobs), rng.integers(0, W, n_blobs)] = rng.uniform(0.5, 1.0, n_blobs)
    canvas = ndimage.gaussian_filter(canvas, 1.5)
    canvas = 100.0 + 300.0 * canvas / canvas.max()
    gains = None
    if smooth:
        shifts = np.rint(np.stack([_smooth_path(rng, T, -my, my, smooth), _smooth_path(rng, T, -mx, mx, smooth)], axis=1))
        gains = _smooth_path(rng, T, 0.8, 1.3, smooth)
    elif fractional:
        shifts = np.stack([rng.uniform(-my + 1, my - 1, T), rng.uniform(-mx + 1, mx - 1, T)], axis=1)
    else:
        shifts = np.stack([rng.integers(-my, my + 1, T), rng.integers(-mx, mx + 1, T)], axis=1).astype(np.float64)
        corners = [(0, 0), (-my, -mx), (my, mx), (-my, mx), (my, -mx)]
        shifts[:min(T, len(corners))] = corners[:T]
    if not moving:
        shifts = shifts * 0.0
    base = canvas[M:M + d1, M:M + d2]
    frames = np.empty((T, d1, d2))
    for t in range(T):
        if fractional:
            moved = shift_bilinear(canvas, -shifts[t])[M:M + d1, M:M + d2]
        else:
            sy, sx = int(shifts[t, 0]), int(shifts[t, 1])
            moved = canvas[M - sy:M - sy + d1, M - sx:M - sx + d2]
        frames[t] = (rng.uniform(0.8, 1.3) if gains is None else gains[t]) * moved + noise * rng.standard_normal((d1, d2))
    if np.dtype(dtype) != np.float32:
        info = np.iinfo(dtype)
        frames = np.clip(np.rint(frames), info.min, info.max)
    return frames.astype(dtype), base.astype(np.float32), shifts
