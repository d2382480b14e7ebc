"""The planted movies of the piecewise registration tests (tests/piecewise_ref.planted_piecewise_movie), by name, with the
float64 reference of each: shared between test_piecewise_host, which shows that the reference recovers the planted field
with room, and test_gpu_piecewise, which holds the device to the reference."""
import functools

import numpy as np

from tests import piecewise_ref as Q

PLANTED = {
    # the trial of DESIGN section 4p
    "field": dict(movie=dict(T=12, d1=96, d2=128, max_shift=(5, 5), seed=31), max_deviation=(3, 3), patch=(32, 32),
                  stride=(24, 24)),
    "rigid": dict(movie=dict(T=8, d1=96, d2=128, max_shift=(5, 5), seed=32, piecewise=False), max_deviation=(3, 3),
                  patch=(32, 32), stride=(24, 24)),
    "stream": dict(movie=dict(T=1300, d1=44, d2=60, max_shift=(3, 3), seed=33, rigid=2, deviation=1.5),
                   max_deviation=(2, 2), patch=(16, 20), stride=(12, 14)),
}
# measured with the float64 reference on "field" (DESIGN section 4p): RMS error of the per-pixel field inside ``valid``
FIELD_RMS_PIECEWISE, FIELD_RMS_RIGID = 0.105, 0.323


@functools.lru_cache(maxsize=None)
def planted(name):
    """(movie, base, field) of PLANTED[name]; shared between tests, never written to."""
    mov, base, field = Q.planted_piecewise_movie(**PLANTED[name]["movie"])
    for a in (mov, base, field):
        a.setflags(write=False)
    return mov, base, field


def settings(name):
    """The keyword arguments of register_piecewise / register_piecewise_ref for PLANTED[name]."""
    p = PLANTED[name]
    return dict(max_shift=p["movie"]["max_shift"], max_deviation=p["max_deviation"], patch=p["patch"], stride=p["stride"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """register_piecewise_ref of the planted movie against its base (float64 surfaces), without the warped movie."""
    mov, base, _ = planted(name)
    ref = Q.register_piecewise_ref(mov, base, warp=False, **settings(name))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref
