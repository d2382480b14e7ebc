"""
register_movie and register_piecewise with ``prefilter=`` on the device: the planted one-photon movies of
tests/spatial_ref.py (cells under a large static hill), and the composition law that defines the option: estimating
through the filter is estimating on the filtered movie against the filtered template, and applying to the unfiltered one.
tests/test_spatial_host.py shows in float64 that the planted cases are decidable with room.
"""
import gc

import numpy as np
import pytest

import localmd_amd
from localmd_amd import register as RG
from localmd_amd import spatial as S
from localmd_amd.dataset import lazy_data_loader
from tests import piecewise_planted as PP
from tests import register_ref as R
from tests import spatial_ref as SR
from tests.register_planted import PLANTED, planted

pytestmark = pytest.mark.gpu


class _Counting(lazy_data_loader):
    """A lazy movie over an array; counts how often every frame is served."""

    def __init__(self, a):
        self.a = a
        self.count = np.zeros(len(a), dtype=np.int64)

    dtype = property(lambda self: self.a.dtype)
    shape = property(lambda self: self.a.shape)

    def _compute_at_indices(self, indices):
        idx = np.arange(len(self.a))[indices].reshape(-1)
        np.add.at(self.count, idx, 1)
        return self.a[idx]


def test_explicit_template_needs_the_filter(gpu_ctx):
    """The reason for the feature: against the true template the unfiltered correlation follows the static hill and gets
    (nearly) every frame wrong; through the band-pass every planted shift comes back."""
    mov, tmpl, shifts = SR.one_photon("explicit")
    ms = SR.ONE_PHOTON["explicit"]["max_shift"]
    reg = localmd_amd.register_movie(mov, max_shift=ms, template=tmpl, prefilter=SR.SIGMA, subpixel=False, ctx=gpu_ctx)
    assert np.array_equal(reg.integer_shifts, shifts.astype(np.int32)) and np.array_equal(reg.shifts, shifts)
    assert isinstance(reg.prefilter, S.SpatialFilter) and (reg.prefilter.kind, reg.prefilter.sigma) == ("bandpass", (1.5, 1.5))
    assert reg.template.tobytes() == tmpl.tobytes()
    sub = localmd_amd.register_movie(mov, max_shift=ms, template=tmpl, prefilter=SR.SIGMA, ctx=gpu_ctx)
    assert np.array_equal(sub.integer_shifts, shifts.astype(np.int32)) and np.abs(sub.shifts - shifts).max() <= 0.5
    none = localmd_amd.register_movie(mov, max_shift=ms, template=tmpl, prefilter=None, subpixel=False, ctx=gpu_ctx)
    wrong = int((none.integer_shifts != shifts.astype(np.int32)).any(axis=1).sum())
    print("without the filter:", wrong, "of", len(mov), "frames wrong")
    assert wrong >= 20 and none.prefilter is None


def test_built_template_through_the_filter(gpu_ctx):
    mov, _, shifts = SR.one_photon("built")
    ms = SR.ONE_PHOTON["built"]["max_shift"]
    reg = localmd_amd.register_movie(mov, max_shift=ms, template_frames=200, template_iters=2, prefilter=SR.SIGMA,
                                     subpixel=False, ctx=gpu_ctx)
    assert np.array_equal(reg.integer_shifts, shifts.astype(np.int32))
    # the template is an unfiltered image: it carries the hill, and it reproduces the run
    assert reg.template.shape == mov.shape[1:] and reg.template.mean() > 500
    want = SR.build_template64(mov, S.spatial_filter(SR.SIGMA), ms, 2)
    assert np.abs(reg.template - want).max() <= 1e-5 * np.abs(want).max()
    again = localmd_amd.register_movie(mov, max_shift=ms, template=reg.template, prefilter=reg.prefilter, subpixel=False,
                                       ctx=gpu_ctx)
    assert again.shifts.tobytes() == reg.shifts.tobytes() and again.peak.tobytes() == reg.peak.tobytes()


def test_composition_with_register_movie(gpu_ctx):
    import torch

    mov, tmpl, _ = SR.one_photon("explicit")
    ms = SR.ONE_PHOTON["explicit"]["max_shift"]
    for prefilter in (SR.SIGMA, (1.0, 2.5), S.spatial_filter(2.0, "highpass"), S.spatial_filter(1.0, "lowpass", (2, 3))):
        filt = S.as_filter(prefilter)
        F = localmd_amd.filter_movie(mov, torch.empty(mov.shape, dtype=torch.float32, device=gpu_ctx.device), filt, ctx=gpu_ctx)
        assert R.same_bits(F.cpu().numpy(), S.filter_frames(mov, filt))
        regF = localmd_amd.register_movie(F, max_shift=ms, template=S.filter_frames(tmpl, filt), ctx=gpu_ctx)
        out = np.empty(mov.shape, np.float32)
        reg = localmd_amd.register_movie(mov, out, max_shift=ms, template=tmpl, prefilter=prefilter, ctx=gpu_ctx)
        assert reg.shifts.tobytes() == regF.shifts.tobytes() and reg.peak.tobytes() == regF.peak.tobytes(), filt
        assert np.array_equal(reg.integer_shifts, regF.integer_shifts)
        want = localmd_amd.apply_shifts(mov, np.empty(mov.shape, np.float32), regF.shifts, ctx=gpu_ctx)
        assert R.same_bits(out, want), filt                          # the unfiltered frames are what is shifted
        assert reg.template.tobytes() == tmpl.tobytes() and regF.prefilter is None
        assert reg.prefilter.wy.tobytes() == filt.wy.tobytes() and reg.prefilter.kind == filt.kind


def test_composition_with_register_piecewise(gpu_ctx):
    mov, base, _ = PP.planted("field")
    kw = PP.settings("field")
    hill = SR.hill(*mov.shape[1:])
    mov = (mov.astype(np.float64) + hill).astype(np.float32)
    tmpl = (base.astype(np.float64) + hill).astype(np.float32)
    filt = S.spatial_filter(SR.SIGMA)
    F = S.filter_frames(mov, filt)
    regF = localmd_amd.register_piecewise(F, template=S.filter_frames(tmpl, filt), ctx=gpu_ctx, **kw)
    out = np.empty(mov.shape, np.float32)
    reg = localmd_amd.register_piecewise(mov, out, template=tmpl, prefilter=SR.SIGMA, ctx=gpu_ctx, **kw)
    assert reg.shifts.tobytes() == regF.shifts.tobytes() and np.array_equal(reg.fallback, regF.fallback)
    assert reg.rigid.shifts.tobytes() == regF.rigid.shifts.tobytes() and reg.peak.tobytes() == regF.peak.tobytes()
    assert np.any(reg.shifts != reg.rigid.shifts[:, None, None, :]), "the case has no patch that deviates"
    want = localmd_amd.apply_field(mov, np.empty(mov.shape, np.float32), regF, ctx=gpu_ctx)
    assert R.same_bits(out, want)
    assert reg.template.tobytes() == tmpl.tobytes() and reg.prefilter is reg.rigid.prefilter and reg.prefilter.kind == "bandpass"
    assert regF.prefilter is None
    # the filter is what makes the patches decidable under the hill: without it the rigid step is already off
    plain = localmd_amd.register_piecewise(mov, template=tmpl, ctx=gpu_ctx, **kw)
    assert np.abs(plain.rigid.shifts - reg.rigid.shifts).max() > 1


@pytest.fixture(scope="module")
def long_movie():
    """1100 frames (two 1024-frame blocks) of the explicit-template case, cropped to 40 x 56; read-only."""
    mov, tmpl, _ = SR.one_photon("explicit")
    m = np.ascontiguousarray(np.tile(mov[:, :40, :56], (46, 1, 1))[:1100])
    t = np.ascontiguousarray(tmpl[:40, :56])
    m.setflags(write=False)
    return m, t


def test_same_bits_over_batch_sizes_and_sources_and_one_read(gpu_ctx, long_movie):
    import torch

    mov, tmpl = long_movie
    ms = (4, 5)
    kw = dict(max_shift=ms, prefilter=SR.SIGMA, border=100.0, ctx=gpu_ctx)

    def run(movie, **more):
        out = np.empty(mov.shape, np.float32)
        reg = localmd_amd.register_movie(movie, out, **more, **kw)
        return reg.shifts.tobytes(), reg.peak.tobytes(), reg.template.tobytes(), out.tobytes()

    want = run(mov, template=tmpl, frame_batch_size=10000)
    built = run(mov, template_frames=60, frame_batch_size=10000)
    for fbs in (1024, 2048):
        assert run(mov, template=tmpl, frame_batch_size=fbs) == want, fbs
        assert run(mov, template_frames=60, frame_batch_size=fbs) == built, fbs
    dev = torch.from_numpy(mov.copy()).to(gpu_ctx.device)
    assert run(dev, template=tmpl) == want and run(dev, template_frames=60, frame_batch_size=1024) == built
    assert run(torch.from_numpy(mov.copy()), template=tmpl, frame_batch_size=1024) == want
    dest = torch.empty(mov.shape, dtype=torch.float32, device=gpu_ctx.device)
    localmd_amd.register_movie(dev, dest, template=tmpl, **kw)
    assert dest.cpu().numpy().tobytes() == want[3]
    # one read of the movie, plus the template's sample in one strided read
    src = _Counting(mov)
    assert run(src, template=tmpl, frame_batch_size=1024) == want and np.all(src.count == 1)
    src = _Counting(mov)
    assert run(src, template_frames=60, frame_batch_size=1024) == built
    expect = np.ones(len(mov), np.int64)
    expect[RG.sample_frames(len(mov), 60)] += 1
    assert np.array_equal(src.count, expect)
    # the piecewise pass on the same movie: batch sizes and sources
    pw = dict(max_shift=ms, max_deviation=2, patch=(16, 20), stride=(12, 14), template=tmpl, prefilter=SR.SIGMA, ctx=gpu_ctx)
    outs = []
    for movie, fbs in ((mov, 10000), (mov, 1024), (dev, 2048)):
        out = np.empty(mov.shape, np.float32)
        reg = localmd_amd.register_piecewise(movie, out, frame_batch_size=fbs, **pw)
        outs.append((reg.shifts.tobytes(), reg.rigid.shifts.tobytes(), out.tobytes()))
    assert outs[0] == outs[1] == outs[2]


def test_device_memory_does_not_grow_with_the_movie(gpu_ctx, long_movie):
    import torch

    mov, tmpl = long_movie
    d1, d2 = mov.shape[1:]
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
        localmd_amd.register_movie(m, out, max_shift=(4, 5), template=tmpl, prefilter=SR.SIGMA, frame_batch_size=1024,
                                   ctx=gpu_ctx)
        peaks[n] = torch.cuda.max_memory_allocated() - start
    kw = dict(d1=d1, d2=d2, nb=1024, esize=4, host_source=True, n_batches=2, my=4, mx=5, out_esize=4, host_dest=True)
    plan = RG.register_device_bytes(prefilter=True, **kw)
    assert peaks[8192] <= peaks[2048] + 4096, peaks
    assert 3 * 1024 * d1 * d2 * 4 <= peaks[2048] <= plan, (peaks, plan)      # two batches and the filtered block
    with pytest.raises(ValueError, match="device memory"):
        localmd_amd.register_movie(np.broadcast_to(mov[:1, :1, :1], (10 ** 7, 1024, 1024)), max_shift=4, prefilter=1.5,
                                   template=np.zeros((1024, 1024), np.float32), frame_batch_size=10 ** 7, ctx=gpu_ctx)


def test_no_filter_is_the_call_without_the_argument(gpu_ctx):
    mov, base, _ = planted("small")
    ms = PLANTED["small"]["max_shift"]
    res = []
    for kw in ({}, dict(prefilter=None)):
        out = np.empty(mov.shape, np.float32)
        reg = localmd_amd.register_movie(mov, out, max_shift=ms, template_frames=20, ctx=gpu_ctx, **kw)
        res.append((reg.shifts.tobytes(), reg.peak.tobytes(), reg.template.tobytes(), out.tobytes(), reg.prefilter))
    assert res[0] == res[1] and res[0][4] is None
    a = localmd_amd.register_piecewise(mov, max_shift=ms, patch=16, stride=12, template=base, ctx=gpu_ctx)
    b = localmd_amd.register_piecewise(mov, max_shift=ms, patch=16, stride=12, template=base, prefilter=None, ctx=gpu_ctx)
    assert a.shifts.tobytes() == b.shifts.tobytes() and a.peak.tobytes() == b.peak.tobytes() and b.prefilter is None


def test_uint16_source_has_the_bits_of_its_fp32_copy(gpu_ctx):
    mov, tmpl, shifts = SR.one_photon("explicit")
    ms = SR.ONE_PHOTON["explicit"]["max_shift"]
    u16 = np.clip(np.rint(mov), 0, 65535).astype(np.uint16)
    res = []
    for m in (u16, u16.astype(np.float32)):
        out = np.empty(mov.shape, np.float32)
        reg = localmd_amd.register_movie(m, out, max_shift=ms, template=tmpl, prefilter=SR.SIGMA, ctx=gpu_ctx)
        built = localmd_amd.register_movie(m, max_shift=ms, template_frames=24, prefilter=SR.SIGMA, ctx=gpu_ctx)
        res.append((reg.shifts.tobytes(), reg.peak.tobytes(), out.tobytes(), built.shifts.tobytes(), built.template.tobytes()))
        assert np.array_equal(reg.integer_shifts, shifts.astype(np.int32))
    assert res[0] == res[1]
