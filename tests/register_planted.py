"""The planted movies of the registration tests (tests/register_ref.planted_movie), by name: every one the GPU tests use
is listed here, so that test_register_host can show that the float64 reference recovers each of its shifts with room."""
import functools

import numpy as np

from tests import register_ref as R

PLANTED = {
    "small": dict(T=40, d1=48, d2=56, max_shift=(4, 4), seed=11, noise=8.0),
    "u16": dict(T=24, d1=40, d2=72, max_shift=(3, 5), seed=12, noise=8.0, dtype=np.uint16),
    "stream": dict(T=2200, d1=24, d2=40, max_shift=(3, 3), seed=13, noise=8.0),
    "e2e": dict(T=400, d1=46, d2=46, max_shift=(3, 3), seed=14, noise=8.0, smooth=40),
}

# the sub-pixel trial of DESIGN section 4o: bilinearly shifted frames, float64 reference
SUBPIXEL_TRIAL = dict(T=200, d1=48, d2=56, max_shift=(4, 4), seed=21, noise=8.0)
SUBPIXEL_WORST = 0.062  # pixels, measured with the trial above (median 0.016)


@functools.lru_cache(maxsize=None)
def planted(name):
    """(movie, base, shifts) of PLANTED[name]; shared between tests, never written to."""
    mov, base, shifts = R.planted_movie(**PLANTED[name])
    for a in (mov, base, shifts):
        a.setflags(write=False)
    return mov, base, shifts
