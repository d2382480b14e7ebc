"""
Offset arithmetic for the tests that reach past 2^31 elements and 2^32 bytes through a stride (test infrastructure only;
tests/test_gpu_large_offsets.py uses it on the device, tests/test_bigbuf_host.py checks it without one).

One buffer of WORDS 4-byte words is viewed as uint16, int16 or float32 and never filled.  A geometry names a few short live
windows in it, the last of which starts past 2^31 elements.  An index computed in 32 bits does not reach such a window: it
lands at the offset modulo 2^31 (a sign bit dropped or an int wrapped and masked), modulo 2^32 (an unsigned wrap) or, when
the byte offset is formed in 32 bits, at the byte offset modulo 2^32.  alias_windows() lists those places.  A test writes
the typed tests' poison there before a read and a sentinel before a write, so a truncated read shows in the result and a
truncated write as a damaged sentinel, instead of going unnoticed in memory nobody looks at.
"""
from collections import namedtuple

WORDS = 2 ** 31 + 2 ** 14          # 4-byte words of the buffer (about 8.6 GB)
STRIDE = 2 ** 30 + 4099            # the row / frame stride of most geometries, in elements
ROW_LIVE = 70                      # live elements per row
FRAME = (12, 12)                   # the frames of the registration entries

# name: what is strided; itemsize: bytes per element of the view; starts: first element of each live window; live: length
Geometry = namedtuple("Geometry", "name itemsize starts live")


def capacity(itemsize):
    """Elements of the buffer seen as a type of `itemsize` bytes."""
    return WORDS * 4 // itemsize


def strided(name, itemsize, count, stride, live, base=0):
    return Geometry(name, itemsize, tuple(base + r * stride for r in range(count)), live)


def live_windows(g):
    return [(s, s + g.live) for s in g.starts]


def alias_windows(g):
    """Where a truncated offset of a live window lands: the element offset mod 2^31 and mod 2^32, and the byte offset mod
    2^32, wherever that is another place than the window itself (sorted, each once)."""
    out = set()
    for s in g.starts:
        for a in (s % 2 ** 31, s % 2 ** 32, (s * g.itemsize % 2 ** 32) // g.itemsize):
            if a != s:
                out.add((a, a + g.live))
    return sorted(out)


def _three(name, live):
    return {f"{name}_{tag}": strided(f"{name}_{tag}", size, 3, STRIDE, live)
            for tag, size in (("u16", 2), ("i16", 2), ("f32", 4))}


GEOMETRIES = {}
# three rows of a movie block, of a knot table or of an output at stride 2^30 + 4099: row 2 starts at 2^31 + 8198
GEOMETRIES.update(_three("rows", ROW_LIVE))
# three frames of 12 x 12 at the same stride
GEOMETRIES.update(_three("frames", FRAME[0] * FRAME[1]))
# the 12 rows of ONE 12 x 12 frame at row_stride = 2^28 + 4099 (the frame stride is then 12 row strides, 6.4 GB of uint16: one
# frame fits the buffer, and only as uint16 / int16): rows 8 .. 11 start past 2^31 elements
ROW_STRIDE = 2 ** 28 + 4099
for _tag in ("u16", "i16"):
    GEOMETRIES[f"imgrows_{_tag}"] = strided(f"imgrows_{_tag}", 2, FRAME[0], ROW_STRIDE, FRAME[1])
# ROI traces and their factors: K = 3 rows of 70 frames (pmd_roi_combine's ldc / ldr / ldd / lde, pmd_hals_sweep's ldc / ldp)
GEOMETRIES["traces_f32"] = strided("traces_f32", 4, 3, STRIDE, ROW_LIVE)
# pmd_roi_gather: three frames of D = 2^30 + 4099 pixels; each ROI lists pixels next to 0, 2^30 and D - 1, so the live
# windows are 3 x 3 short runs.  float32 frames of that length (12.9 GB) do not fit the buffer: uint16 and int16 only.
for _tag in ("u16", "i16"):
    GEOMETRIES[f"roi_{_tag}"] = Geometry(f"roi_{_tag}", 2, tuple(f * STRIDE + c for f in range(3)
                                                                 for c in (0, 2 ** 30 - 4, STRIDE - 8)), 8)
# time-major traces for pmd_oasis_ar1: rows of ldy = 2^20 + 3, five problems wide.  Row 2048 is the first past 2^31 elements
# (by 6144) and the last that fits the buffer, so T = 2049 (a 2050th row would start 1 038 339 elements behind its end).
OASIS_T, OASIS_LD, OASIS_N = 2049, 2 ** 20 + 3, 5
GEOMETRIES["oasis_f32"] = strided("oasis_f32", 4, OASIS_T, OASIS_LD, OASIS_N)
