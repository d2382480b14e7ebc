"""Seeded fuzz of the PMDArray consumers over field-of-view and tile geometry on the GPU: export_movie, extract_traces,
regressor_maps, summary_images, quantile_images, rolling_baseline / dff_movie, project_frames, superpixels, demix and
grow_rois on the synthetic cases of tests/consumer_fuzz.py (one row or column of pixels, fewer than 64 pixels, D % 64 in
{0, 1, 63}, one tile, small and merged tiles, pixels no column touches, a U without tile columns or without any column,
rank 1, T below one slice and at 1023 / 1024 / 1025).  Every (consumer, case) pair makes two assertions:

(a) against the reference, with the bound or the equality that the consumer's own GPU module applies to its one fixture
    (the check_<consumer> of tests/consumer_fuzz.py, which tests/test_consumer_fuzz_host.py tries on the CPU);
(b) bitwise invariance: the same bytes for both drawn frame batch sizes (one does not divide T), for the raw movie as a
    float32 and as a uint16 array, and with host-resident factors and after pmd.to_device().

applies() of tests/consumer_fuzz.py names the pairs that are not run; nothing is skipped in here.  Each test prints
"FUZZ <consumer> <case> <figure>=<error / bound>" for the figures of (a)."""
import numpy as np
import pytest

from tests import consumer_fuzz as F

pytestmark = pytest.mark.gpu
CASES = F.draw_cases()
PAIRS = [(consumer, case) for consumer in F.CONSUMERS for case in CASES if F.applies(consumer, case) is None]
_EXPORTED = {}


def _exported(ctx, case):
    """The float32 panels export_movie writes for the case, once for the module."""
    if case["name"] not in _EXPORTED:
        pmd, _, Y = F.make_case(case)
        _EXPORTED[case["name"]] = F.exported(ctx, pmd, Y)
    return _EXPORTED[case["name"]]


@pytest.mark.parametrize("consumer,case", PAIRS, ids=["{}-{}".format(consumer, case["name"]) for consumer, case in PAIRS])
def test_consumer_on_case(gpu_ctx, consumer, case):
    from localmd_amd import decomposition as Dm

    Dm.QUIET = True
    pmd, _, Y = F.make_case(case)
    small, big = case["fbs"]
    first = F.container(Y, case["container"])
    other = F.container(Y, "uint16" if case["container"] == "float32" else "float32")
    assert first.dtype != other.dtype and np.array_equal(first.astype(np.float32), other.astype(np.float32))
    run = F.RUN[consumer]
    # (a) against the reference
    result = run(gpu_ctx, case, first, big)
    full = dict(result, exported=_exported(gpu_ctx, case)) if consumer in F.NEEDS_EXPORT else result
    figures = {}
    try:
        F.CHECK[consumer](full, case, figures)
    finally:
        for key, ratio in figures.items():
            print("FUZZ", consumer, case["name"], "{}={:.3g}".format(key.replace(" ", "_"), ratio))
    # (b) the same bytes whatever the batch, the container and the residency of the factors
    want = F.bytes_of(result)
    more = {"demixed": result["dm"]} if consumer == "grow" else {}
    if consumer in F.USES_MOVIE:
        assert F.bytes_of(run(gpu_ctx, case, first, small, **more)) == want, ("frame_batch_size", small, big)
        assert F.bytes_of(run(gpu_ctx, case, other, big, **more)) == want, ("container", str(other.dtype))
    pmd.to_device(ctx=gpu_ctx)
    try:
        resident = run(gpu_ctx, case, first, big, resident=True, **more)
    finally:
        pmd.to_host()
    assert F.bytes_of(resident) == want, "device-resident factors"
    if consumer == "export":
        # with pmd[...] of the resident factors against the exported denoised movie on the same frames
        F.check_export(dict(resident, exported=_exported(gpu_ctx, case)), case)
