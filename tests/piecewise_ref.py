"""Plain NumPy / SciPy statements of piecewise-rigid registration (localmd_amd.piecewise, csrc/piecewise.hip), on top of
those of the rigid step (tests/register_ref.py).

Conventions (binding): max_shift = (my, mx), max_deviation = (ey, ex) in 1 .. 7, oy = my + ey, ox = mx + ex.  The patch
area is rows [oy, d1 - oy) x columns [ox, d2 - ox) of the template, Hh x Ww.  Patches are ph x pw (8 .. the area) at
strides 1 <= sy <= ph, 1 <= sx <= pw; row starts a_i = min(i sy, Hh - ph) for i < gy = 1 + ceil((Hh - ph) / sy), columns
the same; t'_p is the fp32 template on patch p minus the patch's own mean (float64, rounded once).  With (cy, cx) the
frame's integer rigid peak, the surface of patch p is
    C[v, u] = sum_{i < ph, j < pw} t'_p[i, j] f[oy + a + i + cy + v - ey, ox + b + j + cx + u - ex],  v <= 2 ey, u <= 2 ex,
= scipy.signal.correlate2d(the (ph + 2 ey) x (pw + 2 ex) sub-image of f at (my + a + cy, mx + b + cx), t'_p, "valid").
Its peak is register_ref.peak's; the patch shift is (cy + dy, cx + dx) + subpixel_peak(neigh); a patch whose surface has
no finite entry, or whose t' is zero, takes the frame's rigid shift.  Patch centres are yc_i = oy + a_i + (ph - 1) / 2;
row y has i0 = the last centre at or before y, clipped to 0 .. max(gy - 2, 0), and the weight
ay = clip((y - yc_i0) / (yc_{i0 + 1} - yc_i0), 0, 1) rounded once to fp32 (0 when gy = 1).  The shift of a pixel is, per
component, top = fl(g00 + fl(ax fl(g01 - g00))), bot the same on the next grid row, s = fl(top + fl(ay fl(bot - top))).
The warp: Y = fl(float(y) + s_y) clamped to [-1, d1] (NaN -> -1), iy = floor(Y), fy = Y - iy, columns the same,
w00 = fl(fl(1 - fy) fl(1 - fx)), w01 = fl(fl(1 - fy) fx), w10 = fl(fy fl(1 - fx)), w11 = fl(fy fx),
out = quant(fl(fl(fl(w00 a) + fl(w01 b)) + fl(fl(w10 c) + fl(w11 d)))), samples and borders as in register_ref.apply_frame.

The patch kernel's summation order and its forward bound.  A patch is cut into tiles of 32 rows x 64 columns.  Inside a
tile the rows fall into K = min(32, 256 // (2 ey + 1)) residue classes (row i is in class i mod K); an accumulator is one
fmaf chain (the product is not rounded) over the rows of its class, then the columns: at most
L = ceil(min(32, ph) / K) min(64, pw) terms.  The K classes are added in ascending order (K - 1 roundings), then the
tiles in ascending order (tiles - 1 roundings).  A term passes through at most n = L + (K - 1) + (tiles - 1) roundings
and |computed - exact| <= gamma_n sum |t'| |f|, gamma_n = n u / (1 - n u), u = 2^-24 (Higham, section 4.2).
"""
import numpy as np
from scipy import ndimage, signal

from tests import register_ref as R

U = 2.0 ** -24


# ---- geometry ----------------------------------------------------------------------------------------------------
def starts(H, p, s):
    g = 1 + -(-(H - p) // s)
    return [min(i * s, H - p) for i in range(g)]


def geometry(d1, d2, max_shift, max_deviation, patch, stride):
    """dict: oy, ox, Hh, Ww, ystart, xstart (lists), yc, xc (float64 arrays), gy, gx."""
    (my, mx), (ey, ex), (ph, pw), (sy, sx) = max_shift, max_deviation, patch, stride
    oy, ox = my + ey, mx + ex
    Hh, Ww = d1 - 2 * oy, d2 - 2 * ox
    ys, xs = starts(Hh, ph, sy), starts(Ww, pw, sx)
    return dict(d1=d1, d2=d2, my=my, mx=mx, ey=ey, ex=ex, ph=ph, pw=pw, oy=oy, ox=ox, Hh=Hh, Ww=Ww, ystart=ys, xstart=xs,
                yc=np.array([oy + a + (ph - 1) / 2 for a in ys]), xc=np.array([ox + b + (pw - 1) / 2 for b in xs]),
                gy=len(ys), gx=len(xs))


def patch_template(template, geo, i, j):
    t = np.asarray(template, dtype=np.float32)
    a, b = geo["oy"] + geo["ystart"][i], geo["ox"] + geo["xstart"][j]
    win = t[a:a + geo["ph"], b:b + geo["pw"]]
    return (win - np.float32(win.astype(np.float64).mean())).astype(np.float32)


def packed_templates(template, geo):
    return np.stack([patch_template(template, geo, i, j) for i in range(geo["gy"]) for j in range(geo["gx"])])


# ---- the surface and its bound -----------------------------------------------------------------------------------
def sub_image(frame, geo, i, j, centre):
    """The (ph + 2 ey) x (pw + 2 ex) pixels of the frame under the surface of patch (i, j) around ``centre`` (clamped to
    the search range, as the kernel clamps it)."""
    cy = int(np.clip(centre[0], -geo["my"], geo["my"]))
    cx = int(np.clip(centre[1], -geo["mx"], geo["mx"]))
    y = geo["my"] + geo["ystart"][i] + cy
    x = geo["mx"] + geo["xstart"][j] + cx
    return np.asarray(frame)[y:y + geo["ph"] + 2 * geo["ey"], x:x + geo["pw"] + 2 * geo["ex"]]


def surface64(frame, tp, geo, i, j, centre):
    """The float64 surface (2 ey + 1, 2 ex + 1) of patch (i, j) of one frame."""
    sub = sub_image(frame, geo, i, j, centre).astype(np.float64)
    return signal.correlate2d(sub, np.asarray(tp, dtype=np.float64), mode="valid")


def roundings(ph, pw, ey):
    """n of the module docstring."""
    K = min(32, 256 // (2 * ey + 1))
    tiles = -(-ph // 32) * -(-pw // 64)
    return -(-min(32, ph) // K) * min(64, pw) + (K - 1) + (tiles - 1)


def forward_bound(frame, tp, geo, i, j, centre):
    """The bound of |fp32 surface - exact surface| per entry."""
    sub = np.abs(sub_image(frame, geo, i, j, centre).astype(np.float64))
    mag = signal.correlate2d(sub, np.abs(np.asarray(tp, dtype=np.float64)), mode="valid")
    nu = roundings(geo["ph"], geo["pw"], geo["ey"]) * U
    return nu / (1.0 - nu) * mag


def frame_surfaces64(frame, tps, geo, centre):
    """(gy, gx, 2 ey + 1, 2 ex + 1) float64."""
    return np.stack([np.stack([surface64(frame, tps[i * geo["gx"] + j], geo, i, j, centre) for j in range(geo["gx"])])
                     for i in range(geo["gy"])])


# ---- the host finish -----------------------------------------------------------------------------------------------
def finish_frame(surfaces, tps, centre, rigid_shift, subpixel=True):
    """(shifts (gy, gx, 2) float64, ints (gy, gx, 2), peaks (gy, gx), fallback (gy, gx)) of one frame from its patch
    surfaces under both fallback rules."""
    gy, gx = surfaces.shape[:2]
    sh, ints = np.zeros((gy, gx, 2)), np.zeros((gy, gx, 2), np.int32)
    pk, fb = np.zeros((gy, gx), surfaces.dtype), np.zeros((gy, gx), bool)
    for i in range(gy):
        for j in range(gx):
            (dy, dx), p, nb = R.peak(surfaces[i, j])
            pk[i, j] = p
            if np.isnan(p) or not np.any(tps[i * gx + j]):
                fb[i, j], sh[i, j], ints[i, j] = True, rigid_shift, centre
                continue
            off = R.subpixel_peak(nb) if subpixel else np.zeros(2)
            ints[i, j] = (centre[0] + dy, centre[1] + dx)
            sh[i, j] = (centre[0] + dy + off[0], centre[1] + dx + off[1])
    return sh, ints, pk, fb


# ---- the field and the warp, operation by operation in fp32 ----------------------------------------------------------
def axis_table(centres, d):
    """(i0 (d,) int, weight (d,) float32) of one axis."""
    c = np.asarray(centres, dtype=np.float64)
    idx, w = np.zeros(d, np.int64), np.zeros(d, np.float32)
    if len(c) == 1:
        return idx, w
    for y in range(d):
        i0 = 0
        while i0 < len(c) - 2 and c[i0 + 1] <= y:
            i0 += 1
        idx[y] = i0
        w[y] = np.float32(min(max((y - c[i0]) / (c[i0 + 1] - c[i0]), 0.0), 1.0))
    return idx, w


def tables(geo):
    return axis_table(geo["yc"], geo["d1"]) + axis_table(geo["xc"], geo["d2"])


def field32(grid, tabs):
    """(d1, d2, 2) float32: the field of one (gy, gx, 2) grid, every operation rounded to fp32."""
    g = np.asarray(grid, dtype=np.float32)
    gy, gx = g.shape[:2]
    ri, rw, ci, cw = tabs
    f32 = np.float32
    out = np.empty((len(ri), len(ci), 2), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for y in range(len(ri)):
            i0 = min(max(int(ri[y]), 0), max(gy - 2, 0))
            i1 = min(i0 + 1, gy - 1)
            j0 = np.clip(np.asarray(ci, dtype=np.int64), 0, max(gx - 2, 0))
            j1 = np.minimum(j0 + 1, gx - 1)
            ax = np.asarray(cw, dtype=np.float32)[:, None]
            top = (g[i0, j0] + (ax * (g[i0, j1] - g[i0, j0]).astype(f32)).astype(f32)).astype(f32)
            bot = (g[i1, j0] + (ax * (g[i1, j1] - g[i1, j0]).astype(f32)).astype(f32)).astype(f32)
            out[y] = (top + (f32(rw[y]) * (bot - top).astype(f32)).astype(f32)).astype(f32)
    return out


def field64(grid, yc, xc, d1, d2):
    """The float64 bilinear interpolation of the grid between the centres, constant beyond the outermost ones."""
    g = np.asarray(grid, dtype=np.float64)
    y, x = np.arange(d1, dtype=np.float64), np.arange(d2, dtype=np.float64)
    out = np.empty((d1, d2, 2))
    for k in range(2):
        rows = np.stack([np.interp(x, xc, g[i, :, k]) if len(xc) > 1 else np.full(d2, g[i, 0, k]) for i in range(len(yc))])
        for c in range(d2):
            out[:, c, k] = np.interp(y, yc, rows[:, c]) if len(yc) > 1 else rows[0, c]
    return out


def coordinate(base, s, d):
    with np.errstate(invalid="ignore", over="ignore"):
        Y = (np.asarray(base, np.float32) + np.asarray(s, np.float32)).astype(np.float32)
    out = np.minimum(Y, np.float32(d))
    out[~(Y >= -1)] = -1.0
    return out.astype(np.float32)


def warp_frame(frame, field, border="nearest", dtype=np.float32):
    """One frame sampled at (y + s_y, x + s_x), operation by operation in fp32."""
    f = np.asarray(frame)
    d1, d2 = f.shape
    f32 = np.float32
    constant = not isinstance(border, str)
    fill = f32(border) if constant else None
    Y = coordinate(np.arange(d1, dtype=f32)[:, None], field[..., 0], d1)
    X = coordinate(np.arange(d2, dtype=f32)[None, :], field[..., 1], d2)
    iy, ix = np.floor(Y), np.floor(X)
    fy, fx = (Y - iy).astype(f32), (X - ix).astype(f32)
    iy, ix = iy.astype(np.int64), ix.astype(np.int64)

    def sample(y, x):
        v = f[np.clip(y, 0, d1 - 1), np.clip(x, 0, d2 - 1)].astype(f32)
        if constant:
            v = np.where((y >= 0) & (y < d1) & (x >= 0) & (x < d2), v, fill)
        return v

    a, b, c, d = sample(iy, ix), sample(iy, ix + 1), sample(iy + 1, ix), sample(iy + 1, ix + 1)
    with np.errstate(invalid="ignore", over="ignore"):
        gy_, gx_ = (f32(1) - fy).astype(f32), (f32(1) - fx).astype(f32)
        w00, w01, w10, w11 = (gy_ * gx_).astype(f32), (gy_ * fx).astype(f32), (fy * gx_).astype(f32), (fy * fx).astype(f32)
        top = ((w00 * a).astype(f32) + (w01 * b).astype(f32)).astype(f32)
        bot = ((w10 * c).astype(f32) + (w11 * d).astype(f32)).astype(f32)
        return R.quantize((top + bot).astype(f32), dtype)


def warp_movie(movie, grids, tabs, border="nearest", dtype=np.float32):
    return np.stack([warp_frame(f, field32(np.asarray(g, dtype=np.float32), tabs), border, dtype)
                     for f, g in zip(movie, grids)])


def warp64(frame, field):
    """The float64 bilinear sample of a frame at (y + s_y, x + s_x), edges clamped (map_coordinates, order 1)."""
    d1, d2 = frame.shape
    y = np.clip(np.arange(d1)[:, None] + field[..., 0], 0, d1 - 1)
    x = np.clip(np.arange(d2)[None, :] + field[..., 1], 0, d2 - 1)
    return ndimage.map_coordinates(np.asarray(frame, dtype=np.float64), [y, x], order=1, mode="nearest")


# ---- the whole function ----------------------------------------------------------------------------------------------
def register_piecewise_ref(movie, template, max_shift, max_deviation, patch, stride, subpixel=True, border="nearest",
                           dtype=np.float32, warp=True):
    """dict: rigid (register_ref's dict without its movie), shifts (T, gy, gx, 2) float64, integer_shifts, peak, fallback,
    surfaces (T, gy, gx, 2 ey + 1, 2 ex + 1) float64, geometry, and the corrected movie (``warp``)."""
    T, d1, d2 = np.asarray(movie).shape
    geo = geometry(d1, d2, max_shift, max_deviation, patch, stride)
    tps = packed_templates(template, geo)
    tp = R.window_template(template, *max_shift)
    rig = dict(shifts=[], integer_shifts=[], peak=[], surfaces=[])
    out = dict(shifts=[], integer_shifts=[], peak=[], fallback=[], surfaces=[])
    for f in movie:
        s = R.surface64(f, tp)
        (cy, cx), pk, nb = R.peak(s)
        off = R.subpixel_peak(nb) if subpixel else np.zeros(2)
        rs = np.array([cy + off[0], cx + off[1]])
        for k, v in zip(("shifts", "integer_shifts", "peak", "surfaces"), (rs, (cy, cx), pk, s)):
            rig[k].append(v)
        ps = frame_surfaces64(f, tps, geo, (cy, cx))
        sh, ints, ppk, fb = finish_frame(ps, tps, (cy, cx), rs, subpixel)
        for k, v in zip(("shifts", "integer_shifts", "peak", "fallback", "surfaces"), (sh, ints, ppk, fb, ps)):
            out[k].append(v)
    res = {k: np.array(v) for k, v in out.items()}
    res["rigid"] = {k: np.array(v) for k, v in rig.items()}
    res["geometry"] = geo
    if warp:
        res["movie"] = warp_movie(movie, res["shifts"], tables(geo), border, dtype)
    return res


def peak_gap(surface):
    """The peak of a surface minus its runner-up."""
    s = np.sort(np.asarray(surface, dtype=np.float64).reshape(-1))
    return s[-1] - s[-2]


# ---- the planted movie -----------------------------------------------------------------------------------------------
def planted_piecewise_movie(T, d1, d2, max_shift, seed, rigid=3, deviation=2.0, noise=8.0, dtype=np.float32,
                            piecewise=True):
    """(movie (T, d1, d2), base (d1, d2) float32, field (T, d1, d2, 2) float64): the blob canvas of
    register_ref.planted_movie (about 100 .. 400 in value), every frame drawn through its own motion: an integer rigid
    part in -rigid .. rigid per axis plus a smooth deviation of at most ``deviation`` pixels, an offset, a stretch and a
    shear per axis, (0.25 a0 + 0.375 a1 v + 0.375 a2 h) deviation with a in [-1, 1] and v, h in [-1, 1] the normalised
    coordinates; its own gain in 0.8 .. 1.3 and additive Gaussian noise.  The frame is f(q) = canvas(q - w(q)), sampled
    by cubic splines; ``field`` is the true correction s with f(p + s(p)) = base(p), the fixed point of s = w(p + s).
    ``piecewise=False``: the rigid parts alone."""
    my, mx = max_shift
    rng = np.random.default_rng(seed)
    M = max(my, mx) + 4
    H, W = d1 + 2 * M, d2 + 2 * M
    canvas = np.zeros((H, W))
    n_blobs = max(12, H * W // 60)
    canvas[rng.integers(0, H, n_blobs), rng.integers(0, W, n_blobs)] = rng.uniform(0.5, 1.0, n_blobs)
    canvas = ndimage.gaussian_filter(canvas, 1.5)
    canvas = 100.0 + 300.0 * canvas / canvas.max()
    base = canvas[M:M + d1, M:M + d2]
    yy, xx = np.meshgrid(np.arange(d1, dtype=np.float64), np.arange(d2, dtype=np.float64), indexing="ij")
    frames, fields = np.empty((T, d1, d2)), np.empty((T, d1, d2, 2))
    for t in range(T):
        r = rng.integers(-rigid, rigid + 1, 2).astype(np.float64)
        co = rng.uniform(-1, 1, (2, 3)) * (deviation if piecewise else 0.0)

        def w(y, x):
            v, h = 2 * y / (d1 - 1) - 1, 2 * x / (d2 - 1) - 1
            return [r[k] + 0.25 * co[k, 0] + 0.375 * co[k, 1] * v + 0.375 * co[k, 2] * h for k in range(2)]

        wy, wx = w(yy, xx)
        moved = ndimage.map_coordinates(canvas, [M + yy - wy, M + xx - wx], order=3, mode="nearest")
        frames[t] = rng.uniform(0.8, 1.3) * moved + noise * rng.standard_normal((d1, d2))
        sy, sx = wy, wx
        for _ in range(20):
            sy, sx = w(yy + sy, xx + sx)
        fields[t, ..., 0], fields[t, ..., 1] = sy, sx
    if np.dtype(dtype) != np.float32:
        info = np.iinfo(dtype)
        frames = np.clip(np.rint(frames), info.min, info.max)
    return frames.astype(dtype), base.astype(np.float32), fields


def field_rms(est, truth, valid):
    """RMS over frames, the pixels of ``valid`` = (y0, y1, x0, x1) and both components of est - truth."""
    y0, y1, x0, x1 = valid
    d = (np.asarray(est, dtype=np.float64) - truth)[:, y0:y1, x0:x1]
    return float(np.sqrt(np.mean(d ** 2)))
