"""
pmd_spatial_filter and filter_movie on the device (csrc/spatial.hip, localmd_amd/spatial.py).

The kernel against the float32 statement of its contract (spatial.filter_frames) bit for bit: frame sizes around the
32 x 64 tile, radii 0 .. 32, batches, padded strides, unaligned pointers, every pair of element types with saturating
16-bit outputs, the three kinds, NaN and infinities; against float64 within tests/spatial_ref.forward_bound; every
refusal; the launch split past 32 768 frames; a frame stride that reaches past 2^31 elements; the context's stream.  Then
filter_movie over its sources, destinations and batch sizes, its single read, its memory and its failure path.
"""
import ctypes as C
import gc

import numpy as np
import pytest

import localmd_amd
from localmd_amd import spatial as S
from localmd_amd._lib import Context, PMDLibraryError, ptr
from localmd_amd.dataset import TiffArray, lazy_data_loader
from tests import bigbuf as B
from tests import register_ref as R
from tests import spatial_ref as SR

pytestmark = pytest.mark.gpu
_ELEM = {"float32": 0, "uint16": 1, "int16": 2}
_FILL = {"float32": np.nan, "uint16": 65535, "int16": -32768}      # paddings of an input: they would show up
_KEEP = 77                                                          # paddings of an output: they must stay


def _dev(ctx, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _host_ptr(a):
    return C.c_void_p(a.ctypes.data)


def _filter(ctx, frames, filt, dst="float32", pad=(0, 0, 0, 0), offset=(0, 0)):
    """pmd_spatial_filter; pad = extra elements per input row, input frame, output row, output frame; offset = elements
    the input and the output start behind their (256-byte aligned) allocations."""
    import torch

    n, d1, d2 = frames.shape
    rs, ors = d2 + pad[0], d2 + pad[2]
    fs, ofs = d1 * rs + pad[1], d1 * ors + pad[3]
    buf = np.full(offset[0] + n * fs + 8, _FILL[frames.dtype.name], dtype=frames.dtype)
    for k in range(n):
        buf[offset[0] + k * fs:offset[0] + k * fs + d1 * rs].reshape(d1, rs)[:, :d2] = frames[k]
    xd = _dev(ctx, buf.view(np.int16) if buf.dtype == np.uint16 else buf)
    out = torch.from_numpy(np.full(offset[1] + n * ofs + 3, _KEEP, dtype=np.dtype(dst).name.replace("uint16", "int16"))
                           ).to(ctx.device)
    esz, osz = frames.dtype.itemsize, np.dtype(dst).itemsize
    ctx.call("pmd_spatial_filter", C.c_void_p(xd.data_ptr() + offset[0] * esz), _ELEM[frames.dtype.name], fs, rs, n, d1, d2,
             filt.ry, filt.rx, _host_ptr(filt.wy), _host_ptr(filt.wx), filt.centre, filt.box,
             C.c_void_p(out.data_ptr() + offset[1] * osz), _ELEM[np.dtype(dst).name], ofs, ors)
    ctx.sync()
    o = out.cpu().numpy()
    rest = [o[:offset[1]], o[offset[1] + n * ofs:]]
    o = o[offset[1]:]
    got = np.empty((n, d1, d2), dtype=o.dtype)
    for k in range(n):
        img = o[k * ofs:k * ofs + d1 * ors].reshape(d1, ors)
        got[k] = img[:, :d2]
        rest += [img[:, d2:].reshape(-1), o[k * ofs + d1 * ors:(k + 1) * ofs]]
    assert np.all(np.concatenate(rest) == _KEEP), "the kernel wrote outside its frames"
    return got.view(np.dtype(dst))


def _frames(rng, src, shape, scale=500.0):
    if src == "float32":
        return (1000.0 + scale * rng.standard_normal(shape)).astype(np.float32)
    if src == "uint16":
        return rng.integers(0, 65536, shape).astype(np.uint16)
    return rng.integers(-32768, 32768, shape).astype(np.int16)


# around the 32 x 64 tile; (33, 200) has tiles none of whose taps are reflected (the kernel's pointer path) at every radius,
# and at 160 columns the tile at column 64 is such a tile for rx = 32 with its last tap on the last column, at 159 it is not
_SIZES = [(1, 1), (8, 8), (31, 63), (32, 64), (33, 65), (70, 130), (33, 200), (5, 159), (5, 160)]
_RADII = [(0, 0), (1, 1), (3, 3), (7, 7), (32, 32), (0, 5), (7, 1), (32, 3), (2, 32)]


@pytest.mark.parametrize("size", _SIZES, ids=lambda s: "{}x{}".format(*s))
def test_bit_for_bit_around_the_tile_over_radii_and_kinds(gpu_ctx, size):
    d1, d2 = size
    rng = np.random.default_rng(d1 * 1000 + d2)
    frames = _frames(rng, "float32", (2, d1, d2))
    done = 0
    for ry, rx in _RADII:
        if ry > d1 or rx > d2:
            continue
        for kind in S.KINDS:
            filt = S.spatial_filter((0.5 + ry / 2.0, 0.5 + rx / 2.0), kind, (ry, rx))
            got = _filter(gpu_ctx, frames, filt)
            want = S.filter_frames(frames, filt)
            assert R.same_bits(got, want), (size, ry, rx, kind, np.abs(got - want).max())
            err, bound = np.abs(got - SR.filter64(frames, filt)), SR.forward_bound(frames, filt)
            assert np.all(err <= bound), (size, ry, rx, kind, (err / bound).max())
            done += 1
    # the radius equal to the side, both ways
    filt = S.spatial_filter(3.0, "bandpass", (min(d1, 32), min(d2, 32)))
    assert R.same_bits(_filter(gpu_ctx, frames, filt), S.filter_frames(frames, filt))
    assert done >= 3


@pytest.mark.parametrize("n", [1, 2, 65])
def test_batches_strides_and_unaligned_pointers(gpu_ctx, n):
    rng = np.random.default_rng(40 + n)
    frames = _frames(rng, "float32", (n, 33, 200))                   # edge tiles and tiles without a reflected tap
    filt = S.spatial_filter((1.5, 2.5))
    want = S.filter_frames(frames, filt)
    assert R.same_bits(_filter(gpu_ctx, frames, filt), want)
    assert R.same_bits(_filter(gpu_ctx, frames, filt, pad=(3, 5, 1, 9)), want)
    assert R.same_bits(_filter(gpu_ctx, frames, filt, offset=(1, 1)), want)
    assert R.same_bits(_filter(gpu_ctx, frames, filt, pad=(1, 0, 0, 7), offset=(3, 1)), want)
    # a frame alone has the bits it has inside the batch
    k = n // 2
    assert R.same_bits(_filter(gpu_ctx, frames[k:k + 1], filt)[0], want[k])
    u16 = _frames(rng, "uint16", (n, 33, 200))
    assert R.same_bits(_filter(gpu_ctx, u16, filt, "int16", pad=(1, 3, 5, 7), offset=(1, 3)), S.filter_frames(u16, filt, "int16"))


@pytest.mark.parametrize("src", list(_ELEM))
@pytest.mark.parametrize("dst", list(_ELEM))
def test_every_pair_of_element_types(gpu_ctx, src, dst):
    rng = np.random.default_rng(7)
    frames = _frames(rng, src, (3, 37, 200), scale=40000.0)
    seen = set()
    for filt in (S.spatial_filter(1.5, "lowpass"), S.spatial_filter(1.5, "bandpass"), S.spatial_filter((1.0, 2.0), "highpass"),
                 S.SpatialFilter([3.0], [1.0, -2.0, 1.0], centre=-2.0, box=0.5)):
        got = _filter(gpu_ctx, frames, filt, dst)
        want = S.filter_frames(frames, filt, dst)
        assert got.dtype == np.dtype(dst) and R.same_bits(got, want), (src, dst, filt)
        # the input's type matters through its values only
        assert R.same_bits(got, S.filter_frames(frames.astype(np.float32), filt, dst))
        seen |= set(np.unique(want).tolist()) if dst != "float32" else set()
    if dst != "float32":
        info = np.iinfo(dst)
        assert info.min in seen and info.max in seen, "the case does not saturate on both sides"


def test_nan_and_inf_pixels(gpu_ctx):
    rng = np.random.default_rng(8)
    frames = _frames(rng, "float32", (2, 40, 200))
    frames[0, 10, 12], frames[0, 10, 100], frames[0, 30, 30], frames[1, 0, 0], frames[1, 39, 199] = np.nan, np.inf, -np.inf, np.inf, np.nan
    for kind, radius in (("lowpass", (2, 5)), ("bandpass", (3, 4)), ("highpass", (4, 0)), ("lowpass", (0, 0))):
        filt = S.spatial_filter(2.0, kind, radius)
        got, want = _filter(gpu_ctx, frames, filt), S.filter_frames(frames, filt)
        assert R.same_bits(got, want), kind
        assert (~np.isfinite(got)).sum() >= 5
        for dst in ("uint16", "int16"):
            assert R.same_bits(_filter(gpu_ctx, frames, filt, dst), S.filter_frames(frames, filt, dst)), (kind, dst)
    # a window's worth of pixels around a NaN, no more (the host test pins the emulation's extent)
    filt = S.spatial_filter(2.0, "lowpass", (2, 5))
    assert np.isnan(_filter(gpu_ctx, frames[:1], filt)[0]).sum() == 5 * 11


def test_dyadic_weights_on_small_integers_are_exact(gpu_ctx):
    rng = np.random.default_rng(5)
    img = rng.integers(-200, 200, (2, 13, 17))
    w = np.array([0.25, 0.5, 0.25], np.float32)
    p = np.pad(img, ((0, 0), (1, 1), (1, 1)), mode="symmetric").astype(np.int64)
    acc, tot = np.zeros(img.shape, np.int64), np.zeros(img.shape, np.int64)
    for i in range(3):
        for j in range(3):
            acc += (1, 2, 1)[i] * (1, 2, 1)[j] * p[:, i:i + 13, j:j + 17]
            tot += p[:, i:i + 13, j:j + 17]
    for centre, box in ((0.0, 0.0), (2.0, 0.0), (0.0, 0.125), (-1.0, 0.5)):
        want = centre * img + acc / 16.0 - box * tot
        for src in ("float32", "int16"):
            got = _filter(gpu_ctx, img.astype(src), S.SpatialFilter(w, w, centre, box))
            assert np.array_equal(got.astype(np.float64), want), (centre, box, src)


def test_rejects_bad_arguments(gpu_ctx):
    import torch

    d1, d2 = 6, 9
    x = torch.zeros(2 * 60, dtype=torch.float32, device=gpu_ctx.device)
    out = torch.full((2 * 60,), 4.0, dtype=torch.float32, device=gpu_ctx.device)
    wy, wx = np.full(5, 0.2, np.float32), np.full(3, 1 / 3, np.float32)
    big = np.full(65, 1 / 65, np.float32)
    names = ["X", "elem", "fs", "rs", "n", "d1", "d2", "ry", "rx", "wy", "wx", "centre", "box", "out", "out_elem", "ofs", "ors"]
    good = [ptr(x), 0, 60, 10, 2, d1, d2, 2, 1, _host_ptr(wy), _host_ptr(wx), 0.0, 0.0, ptr(out), 0, 60, 10]
    for kw in (dict(n=-1), dict(d1=0), dict(d2=0), dict(d1=16385), dict(d2=16385), dict(elem=3), dict(elem=-1), dict(out_elem=3),
               dict(ry=-1), dict(rx=-1), dict(ry=7, wy=_host_ptr(big)), dict(rx=10, wx=_host_ptr(big)),
               dict(ry=33, wy=_host_ptr(big)), dict(rx=33, wx=_host_ptr(big)), dict(rs=8), dict(ors=8), dict(fs=58),
               dict(ofs=58), dict(X=None), dict(wy=None), dict(wx=None), dict(out=None), dict(out=ptr(x)),
               dict(out=C.c_void_p(x.data_ptr() + 4 * 30))):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        with pytest.raises(PMDLibraryError, match=r"failed \(-2\)"):
            gpu_ctx.call("pmd_spatial_filter", *a)
    gpu_ctx.sync()
    assert bool((out == 4.0).all())
    assert gpu_ctx.lib.pmd_spatial_filter(None, *good) == -2
    gpu_ctx.call("pmd_spatial_filter", *[0 if k == "n" else v for k, v in zip(names, good)])
    gpu_ctx.sync()
    assert bool((out == 4.0).all())
    gpu_ctx.call("pmd_spatial_filter", *good)
    gpu_ctx.sync()
    o = out.cpu().numpy().reshape(2, 6, 10)
    assert np.all(o[:, :, :9] == 0) and np.all(o[:, :, 9] == 4.0)
    # the radius may equal the side
    a = list(good)
    a[names.index("ry")], a[names.index("wy")] = 6, _host_ptr(big)
    gpu_ctx.call("pmd_spatial_filter", *a)
    gpu_ctx.sync()


def test_past_the_launch_split(gpu_ctx):
    """65 537 frames of 8 x 8: the launcher cuts the batch at 32 768 frames; every frame has the bits it has alone."""
    rng = np.random.default_rng(9)
    few = _frames(rng, "int16", (97, 8, 8))
    frames = few[np.arange(65537) % 97]
    filt = S.spatial_filter(1.0)
    got = _filter(gpu_ctx, frames, filt, pad=(0, 0, 0, 1))
    want = S.filter_frames(few, filt)
    assert R.same_bits(got, want[np.arange(65537) % 97])
    assert R.same_bits(got[[0, 32767, 32768, 65535, 65536]], _filter(gpu_ctx, frames[[0, 32767, 32768, 65535, 65536]], filt))


# ---- a frame stride past 2^31 elements -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def strided_buffer(gpu_ctx):
    """An int16 buffer that holds three 12 x 12 frames at the frame stride of tests/bigbuf.py (2^30 + 4099 elements, the
    last frame starting at element 2^31 + 8198): 4.3 GB, never filled."""
    import torch

    n = 2 * B.STRIDE + B.FRAME[0] * B.FRAME[1] + 16
    free, _ = torch.cuda.mem_get_info(gpu_ctx.device)
    if free < 2 * n + (1 << 30):
        pytest.skip("less than {:.1f} GB of device memory free".format((2 * n + (1 << 30)) / 1e9))
    buf = torch.empty(n, dtype=torch.int16, device=gpu_ctx.device)
    yield buf
    del buf
    torch.cuda.empty_cache()


def _windows(buf, geo):
    import torch

    return torch.as_strided(buf, (len(geo.starts), geo.live), (B.STRIDE, 1), geo.starts[0])


@pytest.mark.parametrize("src", ["uint16", "int16"])
def test_input_frame_stride_past_2_31_elements(gpu_ctx, strided_buffer, src):
    geo = B.GEOMETRIES["frames_u16" if src == "uint16" else "frames_i16"]
    assert geo.starts[2] > 2 ** 31 and geo.starts[2] + geo.live <= strided_buffer.numel()
    d1, d2 = B.FRAME
    frames = _frames(np.random.default_rng(12), src, (3, d1, d2))
    for a, b in B.alias_windows(geo):                                # where an offset truncated to 32 bits would read
        assert b <= strided_buffer.numel()
        strided_buffer[a:b] = int(np.array(_FILL[src], dtype=src).view(np.int16))
    _windows(strided_buffer, geo).copy_(_dev(gpu_ctx, frames.reshape(3, -1).view(np.int16)))
    import torch

    out = torch.full((3, d1 * d2 + 5), -7777.0, device=gpu_ctx.device)
    filt = S.spatial_filter(1.5)
    gpu_ctx.call("pmd_spatial_filter", ptr(strided_buffer), _ELEM[src], B.STRIDE, d2, 3, d1, d2, filt.ry, filt.rx,
                 _host_ptr(filt.wy), _host_ptr(filt.wx), filt.centre, filt.box, ptr(out), 0, d1 * d2 + 5, d2)
    gpu_ctx.sync()
    got = out.cpu().numpy()
    assert R.same_bits(got[:, :d1 * d2].reshape(3, d1, d2), S.filter_frames(frames, filt)), "a frame was read at a truncated offset"
    assert np.all(got[:, d1 * d2:] == -7777.0)


def test_output_frame_stride_past_2_31_elements(gpu_ctx, strided_buffer):
    geo = B.GEOMETRIES["frames_i16"]
    d1, d2 = B.FRAME
    frames = _frames(np.random.default_rng(13), "float32", (3, d1, d2))
    xd = _dev(gpu_ctx, frames)
    _windows(strided_buffer, geo).fill_(-7777)
    for a, b in B.alias_windows(geo):
        strided_buffer[a:b] = -7777
    filt = S.spatial_filter(1.5, "lowpass")
    gpu_ctx.call("pmd_spatial_filter", ptr(xd), 0, d1 * d2, d2, 3, d1, d2, filt.ry, filt.rx, _host_ptr(filt.wy),
                 _host_ptr(filt.wx), filt.centre, filt.box, ptr(strided_buffer), 2, B.STRIDE, d2)
    gpu_ctx.sync()
    for a, b in B.alias_windows(geo):
        assert bool((strided_buffer[a:b] == -7777).all()), "a frame was written at a truncated offset"
    got = _windows(strided_buffer, geo).cpu().numpy().reshape(3, d1, d2)
    assert np.array_equal(got, S.filter_frames(frames, filt, "int16"))


# ---- the context's stream -------------------------------------------------------------------------------------------
def test_call_runs_on_the_contexts_stream(gpu_ctx):
    """The pattern of tests/test_gpu_abi_conventions.py: a context made under a side stream; the side stream is held by a
    delay, then the input is overwritten with its final values on that stream, then the call is made.  Only a kernel that
    waits behind both on the side stream sees the final values."""
    import torch

    side = torch.cuda.Stream(device=gpu_ctx.device)
    with torch.cuda.stream(side):
        ctx = Context(0)
    try:
        with torch.cuda.stream(side):                                # the ticks of a 40 ms delay (the second probe: warm)
            for _ in range(2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                torch.cuda._sleep(20_000_000)
                e1.record()
                e1.synchronize()
        cycles = int(20_000_000 * 40.0 / e0.elapsed_time(e1))
        rng = np.random.default_rng(14)
        a, b = _frames(rng, "float32", (2, 3, 33, 70))
        filt = S.spatial_filter(1.5)
        final, x = _dev(gpu_ctx, a), _dev(gpu_ctx, b)
        out = torch.zeros_like(x)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(cycles)
            ev = torch.cuda.Event()
            ev.record()
            x.copy_(final, non_blocking=True)
            S.run_filter(ctx, filt, ptr(x), 0, 3, 33, 70, ptr(out))
            pending = not ev.query()
        assert pending, "inconclusive: the delay had ended before the call was made"
        side.synchronize()
        assert R.same_bits(out.cpu().numpy(), S.filter_frames(a, filt)), "the kernel did not wait on the context's stream"
    finally:
        ctx.close()


# ---- filter_movie ---------------------------------------------------------------------------------------------------
class _Counting(lazy_data_loader):
    """A lazy movie over an array; counts how often every frame is served."""

    def __init__(self, a, fail_after=None):
        self.a, self.fail_after, self.served = a, fail_after, 0
        self.count = np.zeros(len(a), dtype=np.int64)

    dtype = property(lambda self: self.a.dtype)
    shape = property(lambda self: self.a.shape)

    def _compute_at_indices(self, indices):
        idx = np.arange(len(self.a))[indices].reshape(-1)
        self.served += len(idx)
        if self.fail_after is not None and self.served > self.fail_after:
            raise OSError("the disk went away")
        np.add.at(self.count, idx, 1)
        return self.a[idx]


@pytest.fixture(scope="module")
def short_movie():
    """1100 frames of 20 x 140 uint16 (two 1024-frame blocks; three tiles a row), its filter and the host's result;
    read-only."""
    rng = np.random.default_rng(21)
    mov = rng.integers(0, 4000, (1100, 20, 140)).astype(np.uint16)
    filt = S.spatial_filter((1.0, 1.5))
    want = S.filter_frames(mov, filt)
    for a in (mov, want):
        a.setflags(write=False)
    return mov, filt, want


def test_filter_movie_sources_destinations_and_batch_sizes(gpu_ctx, tmp_path, short_movie):
    import torch
    from localmd_amd._minitiff import TiffWriter

    mov, filt, want = short_movie
    T, d1, d2 = mov.shape
    for fbs in (1, 1000, 10000):
        got = localmd_amd.filter_movie(mov, np.empty(want.shape, np.float32), filt, frame_batch_size=fbs, ctx=gpu_ctx)
        assert R.same_bits(got, want), fbs
    got = localmd_amd.filter_movie(mov, np.empty(want.shape, np.float32), (1.0, 1.5), ctx=gpu_ctx)      # a bare sigma
    assert R.same_bits(got, want)
    np.save(tmp_path / "m.npy", mov)
    with TiffWriter(str(tmp_path / "m.tif"), mov.shape, np.uint16) as w:
        w.write(mov)
    counting = _Counting(mov)
    i16 = mov.astype(np.int16)                                       # the values are below 2^15: the same frames as int16
    sources = {"memmap": np.load(tmp_path / "m.npy", mmap_mode="r"), "tiff": TiffArray(str(tmp_path / "m.tif")),
               "cpu": torch.from_numpy(i16.copy()), "device": torch.from_numpy(i16.copy()).to(gpu_ctx.device), "lazy": counting}
    for key, src in sources.items():
        got = localmd_amd.filter_movie(src, np.empty(want.shape, np.float32), filt, frame_batch_size=1024, ctx=gpu_ctx)
        assert R.same_bits(got, want), key
    assert np.all(counting.count == 1), "the movie is read once"
    dev = torch.empty(want.shape, dtype=torch.float32, device=gpu_ctx.device)
    assert localmd_amd.filter_movie(sources["device"], dev, filt, ctx=gpu_ctx) is dev
    assert R.same_bits(dev.cpu().numpy(), want)
    localmd_amd.filter_movie(mov, dev.zero_(), filt, frame_batch_size=1024, ctx=gpu_ctx)
    assert R.same_bits(dev.cpu().numpy(), want)
    cpu = torch.empty(want.shape, dtype=torch.float32)
    localmd_amd.filter_movie(mov, cpu, filt, ctx=gpu_ctx)
    assert R.same_bits(cpu.numpy(), want)
    p = localmd_amd.filter_movie(mov, str(tmp_path / "o.npy"), filt, frame_batch_size=1024, ctx=gpu_ctx)
    assert R.same_bits(np.load(p), want)
    localmd_amd.filter_movie(mov, str(tmp_path / "o.tif"), filt, ctx=gpu_ctx)
    assert R.same_bits(TiffArray(str(tmp_path / "o.tif"))[:], want)
    # the other output types and kinds
    for kind, dtype in (("lowpass", "uint16"), ("highpass", "int16")):
        got = localmd_amd.filter_movie(mov, np.empty(want.shape, dtype), 1.2, kind=kind, radius=(2, 4), dtype=dtype,
                                       frame_batch_size=1024, ctx=gpu_ctx)
        assert R.same_bits(got, S.filter_frames(mov, S.spatial_filter(1.2, kind, (2, 4)), dtype)), kind
    # a float32 source
    f32 = mov[:50].astype(np.float32) * np.float32(0.37)
    got = localmd_amd.filter_movie(f32, np.empty(f32.shape, np.float32), filt, ctx=gpu_ctx)
    assert R.same_bits(got, S.filter_frames(f32, filt))


def test_filter_movie_failure_and_aliasing(gpu_ctx, tmp_path, short_movie):
    import torch

    mov, filt, want = short_movie
    for suffix in (".npy", ".tif"):
        p = tmp_path / ("bad" + suffix)
        with pytest.raises(OSError):
            localmd_amd.filter_movie(_Counting(mov, fail_after=1050), str(p), filt, frame_batch_size=1024, ctx=gpu_ctx)
        assert not p.exists()
    dev = torch.from_numpy(want.copy()).to(gpu_ctx.device)
    before = dev.clone()
    for out in (dev, dev[:], dev.view(-1).view(dev.shape)):
        with pytest.raises(ValueError, match="shares memory"):
            localmd_amd.filter_movie(dev, out, filt, ctx=gpu_ctx)
    big = torch.zeros((len(want) + 3,) + want.shape[1:], dtype=torch.float32, device=gpu_ctx.device)
    with pytest.raises(ValueError, match="shares memory"):
        localmd_amd.filter_movie(big[:len(want)], big[3:], filt, ctx=gpu_ctx)
    host = want.copy()
    with pytest.raises(ValueError, match="shares memory"):
        localmd_amd.filter_movie(host, host, filt, ctx=gpu_ctx)
    assert bool((dev == before).all())
    with pytest.raises(ValueError, match="device memory"):          # the bound is checked before anything is allocated
        localmd_amd.filter_movie(np.broadcast_to(mov[:1, :1, :1], (10 ** 6, 4096, 4096)), str(tmp_path / "huge.npy"), filt,
                                 frame_batch_size=10 ** 6, ctx=gpu_ctx)
    assert not (tmp_path / "huge.npy").exists()


def test_filter_movie_memory_does_not_grow_with_the_movie(gpu_ctx, short_movie):
    import torch

    mov, filt, _ = short_movie
    base = np.concatenate([mov, mov])[:2048]
    peaks = {}
    for n in (2048, 8192):
        m = np.concatenate([base] * (n // 2048))
        out = np.empty(m.shape, np.float32)
        gpu_ctx.sync()
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        localmd_amd.filter_movie(m, out, filt, frame_batch_size=1024, ctx=gpu_ctx)
        peaks[n] = torch.cuda.max_memory_allocated() - start
    D = mov.shape[1] * mov.shape[2]
    plan = S.filter_device_bytes(d1=mov.shape[1], d2=mov.shape[2], nb=1024, esize=2, host_source=True, n_batches=2,
                                 out_esize=4, host_dest=True)
    assert peaks[8192] <= peaks[2048] + 4096, peaks
    assert 2 * 1024 * D * 2 <= peaks[2048] <= plan, (peaks, plan)
