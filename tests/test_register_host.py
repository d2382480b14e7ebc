"""Host side of rigid registration (localmd_amd.register) and of its reference (tests/register_ref.py): no device.

The reference surface against a brute-force double loop, subpixel_peak, the host form of the apply step against the
reference's (and against NumPy slicing for integer shifts), argument checks, the memory plan, valid / at_limit,
RegisteredMovie, and the two properties of the method the GPU tests lean on: the float64 reference recovers every
planted integer shift with a gap between the best and the second-best entry above twice the kernel's forward bound
(tests/register_ref.py: PLANTED), and the sub-pixel finish is within SUBPIXEL_WORST pixels of a planted fractional
shift."""
import os

import numpy as np
import pytest

from localmd_amd import register as RG
from localmd_amd.export import quantize
from tests import register_ref as R
from tests.register_planted import PLANTED, SUBPIXEL_TRIAL, SUBPIXEL_WORST, planted


def test_reference_surface_is_the_double_loop():
    rng = np.random.default_rng(0)
    for d1, d2, my, mx in ((12, 13, 2, 1), (10, 11, 1, 1)):
        f = rng.normal(100, 20, (d1, d2)).astype(np.float32)
        tp = R.window_template(rng.normal(100, 20, (d1, d2)), my, mx)
        assert tp.shape == (d1 - 2 * my, d2 - 2 * mx) and tp.dtype == np.float32
        np.testing.assert_allclose(R.surface64(f, tp), R.surface_brute(f, tp, my, mx), rtol=1e-12, atol=1e-9)
        assert RG.window_template(rng.normal(5, 1, (d1, d2)), my, mx).dtype == np.float32


def test_window_template_matches_reference_and_has_zero_mean():
    rng = np.random.default_rng(1)
    t = rng.normal(300, 50, (40, 33)).astype(np.float32)
    a, b = RG.window_template(t, 3, 5), R.window_template(t, 3, 5)
    assert a.tobytes() == b.tobytes() and a.flags.c_contiguous
    assert abs(float(a.astype(np.float64).mean())) < 1e-4


def test_subpixel_peak_exact_parabolas():
    for oy, ox in ((0.0, 0.0), (0.25, -0.4), (-0.5, 0.5), (0.1, 0.3)):
        y, x = np.arange(-1, 2)[:, None], np.arange(-1, 2)[None, :]
        nb = 10.0 - 2.0 * (y - oy) ** 2 - 3.0 * (x - ox) ** 2
        np.testing.assert_allclose(RG.subpixel_peak(nb), (oy, ox), atol=1e-12)
        np.testing.assert_allclose(R.subpixel_peak(nb), (oy, ox), atol=1e-12)
    # a centre that is not the largest of the three (a tie, a skipped NaN): clipped to half a pixel
    nb = np.array([[0, 10.5, 0], [0, 10.0, 0], [0, 1.0, 0]])
    assert RG.subpixel_peak(nb)[0] == -0.5


def test_subpixel_peak_edges_non_finite_and_flat_tops():
    nan = np.nan
    base = np.array([[1.0, 2.0, 1.0], [2.0, 5.0, 4.0], [1.0, 3.0, 1.0]])
    want = R.subpixel_peak(base)
    assert want[0] != 0 and want[1] != 0
    edge_y = base.copy()
    edge_y[0] = nan                                    # the peak lies on the first row of the search range
    assert tuple(RG.subpixel_peak(edge_y)) == (0.0, want[1])
    edge_x = base.copy()
    edge_x[:, 2] = nan
    assert tuple(RG.subpixel_peak(edge_x)) == (want[0], 0.0)
    for bad in (np.inf, -np.inf, nan):
        b = base.copy()
        b[2, 1] = bad
        assert RG.subpixel_peak(b)[0] == 0.0 and RG.subpixel_peak(b)[1] == want[1]
    assert tuple(RG.subpixel_peak(np.full((3, 3), 7.0))) == (0.0, 0.0)           # flat: curvature 0
    up = np.array([[0, 9.0, 0], [0, 5.0, 0], [0, 9.0, 0.0]])                   # curvature positive
    assert RG.subpixel_peak(up)[0] == 0.0
    assert tuple(RG.subpixel_peak(np.full((3, 3), nan))) == (0.0, 0.0)
    # vectorised = one by one
    stack = np.stack([base, edge_y, edge_x, up])
    got = RG.subpixel_peak(stack)
    assert got.shape == (4, 2)
    for k in range(4):
        np.testing.assert_array_equal(got[k], R.subpixel_peak(stack[k]))
    with pytest.raises(ValueError):
        RG.subpixel_peak(np.zeros((3, 2)))


def test_reference_peak_rules():
    s = np.zeros((5, 7), np.float32)
    s[1, 2] = s[3, 4] = 9.0                              # a tie: the first in row-major order
    (dy, dx), pk, nb = R.peak(s)
    assert (dy, dx) == (1 - 2, 2 - 3) and pk == 9.0 and nb[1, 1] == 9.0
    s[0, 0] = np.nan
    s[4, 6] = 10.0
    (dy, dx), pk, nb = R.peak(s)
    assert (dy, dx) == (2, 3) and np.isnan(nb[2]).all() and np.isnan(nb[:, 2]).all() and nb[0, 0] == 0.0
    (dy, dx), pk, nb = R.peak(np.full((3, 3), np.nan, np.float32))
    assert (dy, dx) == (0, 0) and np.isnan(pk) and np.isnan(nb).all()
    (dy, dx), pk, nb = R.peak(np.full((3, 3), -np.inf, np.float32))
    assert (dy, dx) == (0, 0) and np.isnan(pk)


@pytest.mark.parametrize("src", ["float32", "uint16", "int16"])
def test_integer_shifts_are_numpy_slices_bit_for_bit(src):
    rng = np.random.default_rng(2)
    d1, d2 = 9, 11
    mov = rng.integers(-300 if src != "uint16" else 0, 300, (6, d1, d2)).astype(src)
    if src == "float32":
        mov[0, 2, 3], mov[1, 4, 4], mov[2, 0, 0] = np.inf, np.nan, -np.inf
    shifts = np.array([(0, 0), (2, -3), (-1, 4), (3, 3), (-4, -2), (0, 5)], dtype=np.float64)
    got = RG.shift_frames(mov, shifts, border=-7)
    assert got.dtype == mov.dtype and R.same_bits(got, R.apply_movie(mov, shifts, -7.0))
    for k, (dy, dx) in enumerate(shifts.astype(int)):
        want = np.full((d1, d2), -7 if src != "uint16" else 0, dtype=mov.dtype)   # -7 saturates to 0 in uint16
        ys, xs = slice(max(0, -dy), min(d1, d1 - dy)), slice(max(0, -dx), min(d2, d2 - dx))
        want[ys, xs] = mov[k][ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
        assert R.same_bits(got[k], want), k
    near = RG.shift_frames(mov, shifts)                  # nearest: the edge pixel is repeated
    assert R.same_bits(near, R.apply_movie(mov, shifts))
    assert R.same_bits(near[1][:, :3], np.repeat(near[1][:, 3:4], 3, axis=1))
    far = RG.shift_frames(mov[:1], [(100, -100)])        # beyond the frame: the corner pixel everywhere
    assert np.all(far == mov[0, d1 - 1, 0])
    assert np.all(RG.shift_frames(mov[:1], [(100, -100)], border=3) == 3)


@pytest.mark.parametrize("src", ["float32", "uint16", "int16"])
@pytest.mark.parametrize("dst", ["float32", "uint16", "int16"])
def test_apply_emulation_matches_the_reference(src, dst):
    rng = np.random.default_rng(3)
    mov = rng.integers(0, 4000, (7, 10, 12)).astype(src)
    shifts = np.array([(0, 0), (1.5, -2.25), (-0.5, 0.75), (0, 0.5), (2.5, 0), (-3, 2), (11.5, -13.25)])
    for border in ("nearest", 123.5, -5):
        got = RG.shift_frames(mov, shifts, border, dst)
        want = R.apply_movie(mov, shifts, border, dst)
        assert got.dtype == np.dtype(dst) and R.same_bits(got, want), border
    # quantisation is export.quantize: half to even, saturating
    v = np.array([[0.5, 1.5, 2.5, -0.5, 70000.0, -70000.0, np.nan, 3.49]], np.float32)
    assert R.same_bits(R.quantize(v, dst), quantize(v, dst))
    half = np.array([[[1, 2, 4, 7]]], dtype=src)
    got = RG.shift_frames(half, [(0, 0.5)], "nearest", dst)
    assert np.array_equal(got, quantize(np.array([[[1.5, 3.0, 5.5, 7.0]]], np.float32), dst))


def test_shift_tables_and_weights():
    ish, w = RG.shift_tables([(1.25, -0.5), (-3, 2), (-0.75, 0.0)])
    assert ish.dtype == np.int32 and w.dtype == np.float32
    assert ish.tolist() == [[1, -1], [-3, 2], [-1, 0]]
    assert w.tolist() == [[0.375, 0.375, 0.125, 0.125], [1, 0, 0, 0], [0.75, 0, 0.25, 0]]


def test_valid_rectangle_and_at_limit():
    assert RG.valid_rect([(0, 0)], 20, 30) == (0, 20, 0, 30)
    assert RG.valid_rect([(2, -3), (-1, 4)], 20, 30) == (1, 18, 3, 26)
    assert RG.valid_rect([(0.5, -0.25)], 20, 30) == (0, 19, 1, 30)
    assert RG.valid_rect([(25, 0)], 20, 30)[:2] == (0, 0)
    mov = np.arange(4 * 20 * 30, dtype=np.float32).reshape(4, 20, 30)
    sh = np.array([(2, -3), (-1, 4), (0, 0), (1.5, 0.5)])
    out = RG.shift_frames(mov, sh, border=-1.0, dtype="float32")
    y0, y1, x0, x1 = RG.valid_rect(sh, 20, 30)
    assert np.all(out[:, y0:y1, x0:x1] != -1) and y1 - y0 == 17 and x1 - x0 == 23
    for rect in ((y0 - 1, y1, x0, x1), (y0, y1 + 1, x0, x1), (y0, y1, x0 - 1, x1), (y0, y1, x0, x1 + 1)):
        assert np.any(out[:, rect[0]:rect[1], rect[2]:rect[3]] == -1), rect
    reg = RG.Registration(sh, [(2, -3), (-1, 4), (0, 0), (1, 0)], np.ones(4), np.zeros((20, 30)), (2, 4))
    assert reg.at_limit.tolist() == [0, 1] and reg.valid == (y0, y1, x0, x1)
    assert reg.shifts.dtype == np.float64 and reg.integer_shifts.dtype == np.int32 and reg.peak.dtype == np.float32
    assert reg.template.dtype == np.float32 and reg.surfaces is None and "2 at the limit" in repr(reg)


def test_argument_checks_come_before_any_device_work(tmp_path):
    """This machine has no device: anything but the expected error would be a PMDLibraryError from the context."""
    mov = np.zeros((5, 40, 48), np.float32)
    path = str(tmp_path / "x.npy")
    bad = [dict(max_shift=0), dict(max_shift=32), dict(max_shift=(3, 40)), dict(max_shift=(3,)), dict(max_shift=2.5),
           dict(max_shift=True), dict(max_shift=17), dict(max_shift=(17, 20)), dict(template=np.zeros((40, 47))),
           dict(template=np.zeros((40, 48), bool)), dict(template_frames=0), dict(template_iters=-1),
           dict(border="reflect"), dict(border=None), dict(dtype="float64"), dict(dtype="int8"),
           dict(frame_batch_size=0), dict(bigtiff=1)]
    for kw in bad:
        with pytest.raises(ValueError):
            RG.register_movie(mov, path, **kw)
        assert not os.path.exists(path), kw
    with pytest.raises(ValueError):
        RG.register_movie(mov, None, bigtiff=True)
    with pytest.raises(ValueError):
        RG.register_movie(np.zeros((0, 40, 48), np.float32))
    with pytest.raises(ValueError):
        RG.register_movie(np.zeros((40, 48), np.float32))
    with pytest.raises(TypeError):
        RG.register_movie(7)
    with pytest.raises(ValueError):
        RG.register_movie(mov, str(tmp_path / "x.png"))
    with pytest.raises(ValueError):                       # subpixel output is float32
        RG.register_movie(mov.astype(np.uint16), np.zeros((5, 40, 48), np.uint16))
    with pytest.raises(ValueError):
        RG.register_movie(mov, np.zeros((5, 40, 47), np.float32))
    for shifts in (np.zeros((4, 2)), np.zeros((5, 3)), np.full((5, 2), np.nan), np.full((5, 2), 2.0 ** 31),
                   np.zeros((5, 2), bool)):
        with pytest.raises(ValueError):
            RG.apply_shifts(mov, path, shifts)
        assert not os.path.exists(path)
    with pytest.raises(TypeError):
        RG.apply_shifts(mov, None, np.zeros((5, 2)))
    with pytest.raises(ValueError):                       # integer shifts of a uint16 movie are uint16
        RG.apply_shifts(mov.astype(np.uint16), np.zeros((5, 40, 48), np.float32), np.zeros((5, 2)))
    import torch

    for m, o in ((mov, mov), (mov, mov[::-1][::-1]), (torch.from_numpy(mov), torch.from_numpy(mov)[:])):
        with pytest.raises(ValueError, match="shares memory"):
            RG.register_movie(m, o, subpixel=True)
        with pytest.raises(ValueError, match="shares memory"):
            RG.apply_shifts(m, o, np.full((5, 2), 0.5))
    assert RG.check_max_shift(4, 16, 16) == (4, 4) and RG.check_max_shift((1, 31), 10, 70) == (1, 31)
    with pytest.raises(ValueError):
        RG.check_max_shift(5, 17, 40)                     # a 7-row window


def test_memory_plan():
    kw = dict(d1=512, d2=512, nb=10240, esize=2, host_source=True, n_batches=3)
    base = RG.register_device_bytes(**kw)
    assert base >= 2 * 10240 * 512 * 512 * 2
    est = RG.register_device_bytes(my=15, mx=15, n_sample=200, **kw)
    ns, D = 31 * 31, 512 * 512
    tiles = -(-482 // 32) * -(-482 // 64)
    ws = RG.correlate_workspace_bytes(1024, 512, 512, 15, 15)
    assert ws == (RG.WS_TARGET // (4 * tiles * ns)) * 4 * tiles * ns and ws <= RG.WS_TARGET
    assert est - base == 4 * 482 * 482 + ws + 4 * ns * 1024 + 48 * 1024 + 200 * D * 6 + 8 * D
    assert RG.register_device_bytes(my=15, mx=15, n_sample=200, surfaces=True, **kw) - est == 4 * ns * 1024
    host = RG.register_device_bytes(out_esize=4, host_dest=True, **kw)
    assert host - base == 2 * 1024 * D * 4
    assert RG.correlate_workspace_bytes(3, 48, 56, 4, 4) == 3 * 4 * 2 * 81       # 2 tiles, never more than n frames
    # nothing depends on the movie's length: the plan does not take it
    assert RG.register_device_bytes(d1=512, d2=512, nb=10240, esize=2, host_source=False, n_batches=100) < base
    assert RG.sample_frames(1000, 200).size == 200 and RG.sample_frames(7, 200).tolist() == list(range(7))
    s = RG.sample_frames(1000, 200)
    assert s[0] == 0 and s[-1] == 999 and np.all(np.diff(s) >= 4)


def test_registered_movie_is_the_emulation():
    from localmd_amd.dataset import ArrayDataset, lazy_data_loader

    mov, _, planted_shifts = planted("small")
    u16 = np.clip(mov, 0, 65535).astype(np.uint16)
    frac = planted_shifts + np.linspace(-0.4, 0.4, len(mov))[:, None]
    for src, shifts, want_dtype in ((mov, frac, np.float32), (u16, planted_shifts, np.uint16), (u16, frac, np.float32),
                                    (ArrayDataset(u16), frac, np.float32)):
        rm = RG.RegisteredMovie(src, shifts, border=0.0)
        assert isinstance(rm, lazy_data_loader) and rm.shape == mov.shape and rm.dtype == want_dtype
        arr = src._array if isinstance(src, ArrayDataset) else src
        want = R.apply_movie(arr, shifts, 0.0)
        assert R.same_bits(rm[:], want)
        assert R.same_bits(rm[[5, 2, 9]], want[[5, 2, 9]]) and R.same_bits(rm[3:12:4], want[3:12:4])
        assert R.same_bits(rm[7], want[7])
    reg = RG.Registration(frac, np.round(frac), np.ones(len(mov)), mov[0], (4, 4), border=3.0)
    assert R.same_bits(RG.RegisteredMovie(mov, reg)[4], R.apply_frame(mov[4], frac[4], 3.0))
    with pytest.raises(ValueError):
        RG.RegisteredMovie(mov, frac[:-1])


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_float64_reference_recovers_every_planted_shift_with_a_gap(name):
    """What lets the GPU tests demand exact agreement on every frame: the best entry of the float64 surface is the
    planted shift, and it beats the second best by more than twice the kernel's forward bound."""
    mov, base, shifts = planted(name)
    my, mx = PLANTED[name]["max_shift"]
    tp = R.window_template(base, my, mx)
    worst = np.inf
    for t, f in enumerate(mov):
        s = R.surface64(f, tp)
        (dy, dx), pk, _ = R.peak(s)
        assert (dy, dx) == tuple(shifts[t].astype(int)), (name, t)
        second = np.partition(s.reshape(-1), -2)[-2]
        bound = R.forward_bound(f, tp, my, mx).max()
        worst = min(worst, (pk - second) / bound)
        assert pk - second > 2 * bound, (name, t, pk - second, bound)
    print(name, "smallest gap / forward bound:", worst)


def test_subpixel_accuracy_against_the_planted_truth():
    """A property of the method, measured with the float64 reference on bilinearly shifted frames.  The trial of
    DESIGN section 4o gave SUBPIXEL_WORST; 1.5 x it is allowed, as other seeds and SciPy builds move it slightly."""
    kw = dict(SUBPIXEL_TRIAL)
    my, mx = kw["max_shift"]
    mov, base, shifts = R.planted_movie(fractional=True, **kw)
    ref = R.register_ref(mov, base, (my, mx), subpixel=True)
    err = np.abs(ref["shifts"] - shifts)
    print("sub-pixel error: worst", err.max(), "median", np.median(err))
    assert np.all(np.abs(ref["integer_shifts"] - shifts) <= 1.0)
    assert err.max() <= 1.5 * SUBPIXEL_WORST
    whole = R.register_ref(mov, base, (my, mx), subpixel=False)
    assert np.abs(whole["shifts"] - shifts).max() > 2 * err.max()          # the finish is worth having
