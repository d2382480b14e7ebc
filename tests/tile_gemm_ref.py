"""References, case tables, data and launch decisions for the four 64-row tile contractions of csrc/tile_gemm.hip
(tile_atx, tile_xbt, tile_gram, tile_rowmix).  Test infrastructure only: NumPy, no GPU.

  * ref_*:       the contraction in float64, with the same contraction of the absolute values next to it (the error bound
                 of a sum in any order is stated against that one);
  * *_cases():   the tables the GPU tests walk (tests/test_gpu_tile_contractions.py) and the host test proves coverage
                 from (tests/test_tile_gemm_ref.py);
  * exact_data / rounded_data: the two kinds of operands every case runs on;
  * route_of_*:  the launch decisions of pmd_launch_tile_* and pmd_pick_dvariant restated: which kernel instantiation a
                 call reaches, from its shape, leading dimensions, alignment and the route switches of its context;
                 *_launch give the grid facts next to it (K slices, chunks per slice, M blocks, tile passes).
"""
from collections import namedtuple

import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
EXACT_LIMIT = 2 ** 24          # integers below it are fp32 numbers, sums of them in any order too
EXACT_ABS = 7                  # exact operands are integers in [-7, 7]

# contexts by name: the environment a context is created under (tests.util.context_under)
ENVS = {
    "default": {},
    "atx_dma0": {"PMD_ATX_DMA": "0"},
    "gram0": {"PMD_GRAM_MFMA": "0"},
    "rowmix0": {"PMD_ROWMIX_MFMA": "0"},
    "rowmix16": {"PMD_ROWMIX_MFMA": "16"},
    "rowmix64": {"PMD_ROWMIX_MFMA": "64"},
}


def switch(env, name, default):
    return int(ENVS[env].get(name, default))


def round_up(x, m):
    return (x + m - 1) // m * m


def ceil_div(x, m):
    return (x + m - 1) // m


def time_ld(t):
    """pmd_time_ld"""
    return round_up(t, 64) + 64


# pmd_pick_dvariant: (kjw, ks, dpad); the NS template argument of the plain kernel by variant
_DVARIANTS = [(16, 1, 256), (25, 1, 400), (32, 1, 512), (25, 2, 800), (32, 2, 1024), (25, 4, 1600)]
_NS = {(16, 1): 2, (25, 1): 1, (32, 1): 1, (25, 2): 1, (32, 2): 1}


def pick_dvariant(d):
    for v in _DVARIANTS:
        if d <= v[2]:
            return v
    return None


def tile_dpad(d):
    """pmd_tile_dpad"""
    if d > 1024:
        return round_up(d, 1024)
    return pick_dvariant(d)[2]


# ---- launch decisions ------------------------------------------------------------------------------------------------
def atx_launch(d, T, slices):
    """(kz, workgroups along time, chunks per workgroup) of pmd_launch_tile_atx"""
    kz = ceil_div(d, 1024) if d > 1024 else 1
    n_chunks = ceil_div(T, 32)
    slices = min(max(slices, 1), n_chunks)
    cps = ceil_div(n_chunks, slices)
    return kz, ceil_div(n_chunks, cps), cps


def atx_slice_chunks(T, slices):
    """chunks each workgroup along time walks"""
    n_chunks = ceil_div(T, 32)
    _, ny, cps = atx_launch(1, T, slices)
    return [min(n_chunks, (y + 1) * cps) - y * cps for y in range(ny)]


def route_of_atx(d, T, ldx, atx_dma=1, rows=0, rank=None):
    """rows: the hint of pmdk_tile_atx_rows (0: none); rank: the tile's entry of pmd_tiles_project_ranked (None: unranked)"""
    kz = ceil_div(d, 1024) if d > 1024 else 1
    kjw, ks, _ = pick_dvariant(min(d, 1024))
    if (kjw, ks) == (25, 1) and atx_dma and ldx >= 32 * (ceil_div(T, 32) + 2) and ldx % 4 == 0:
        return "tile_atx_dma_kernel<25>" + (":half" if rank is not None and rank <= 32 else "")
    if 0 < rows <= 16 and (kjw, ks) == (32, 2) and kz == 1:
        return "tile_atx_kernel<8,8,1,1>"
    return "tile_atx_kernel<%d,%d,%d>" % (kjw, ks, _NS[(kjw, ks)])


def xbt_launch(d, T, slices):
    """(M tiles per wave, slices with work, frame groups per slice, M blocks) of pmd_launch_tile_xbt"""
    n_groups = ceil_div(T, 16)
    slices = min(max(slices, 1), n_groups)
    gps = ceil_div(n_groups, slices)
    slices = ceil_div(n_groups, gps)
    mtiles = ceil_div(d, 16)
    mpw = 1 if mtiles <= 4 else 2 if mtiles <= 8 else 4 if mtiles <= 16 else 7
    return mpw, slices, gps, ceil_div(mtiles, 4 * mpw)


def route_of_xbt(d):
    return "tile_xbt_lds_kernel<%d>" % xbt_launch(d, 16, 1)[0]


def gram_chunk(length, slices):
    """positions per slice of pmd_launch_tile_gram"""
    return round_up(ceil_div(length, max(slices, 1)), 32)


def route_of_gram(ld, tile_stride, base_aligned=True, gram_mfma=1):
    if gram_mfma and ld % 4 == 0 and ld >= 16 and tile_stride % 4 == 0 and base_aligned:
        return "tile_gram_mfma_kernel"
    return "tile_gram_kernel"


def rowmix_passes(n_tiles):
    """launches of the 32768-tile loop"""
    return ceil_div(n_tiles, 32768)


def route_of_rowmix(n_out, length, ld_in, ld_out, in_tile_stride, out_tile_stride, n_tiles, in_aligned=True, out_aligned=True,
                    rowmix_mfma=-1):
    rm = rowmix_mfma
    quads = (ld_in % 4 == 0 and ld_out % 4 == 0 and in_tile_stride % 4 == 0 and out_tile_stride % 4 == 0 and in_aligned and
             out_aligned and ld_in >= round_up(length, 4) and length >= 4 and rm != 16)
    if n_out > 4 and rm != 0 and quads and (n_tiles >= 8192 or rm == 64):
        return "tile_rowmix_mfma4_kernel"
    if n_out > 4 and rm != 0:
        return "tile_rowmix_mfma_kernel"
    return "tile_rowmix_kernel<%d>" % (4 if n_out <= 4 else 32 if n_out <= 32 else 64)


# ---- float64 references: (value, the same contraction of the absolute values) ------------------------------------------
def _pair(a, b, dtype=np.float64):
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    return np.matmul(a, b), np.matmul(np.abs(a), np.abs(b))


def ref_atx(A, Xg):
    """A (n, 64, d), Xg (n, d, T): the gathered pixel rows -> (n, 64, T)"""
    return _pair(A, Xg)


def ref_xbt(B, Xg):
    """B (n, 64, T), Xg (n, d, T) -> (n, 64, d)"""
    return _pair(B, np.swapaxes(np.asarray(Xg), -1, -2))


# The two kernels below accumulate in fp64 themselves: their rounded cases are compared with the same contraction in
# np.longdouble (dtype argument), so that the reference's own rounding stays far below the bound where the platform's
# long double is wider than a double, and is no worse than the float64 one where it is not.
def ref_gram(In, dtype=np.float64):
    """In (n, 64, len) -> (n, 64, 64)"""
    return _pair(In, np.swapaxes(np.asarray(In), -1, -2), dtype)


def ref_rowmix(N, In, dtype=np.float64):
    """N (n, n_in, n_out), In (n, n_in, len) -> (n, n_out, len)"""
    return _pair(np.swapaxes(np.asarray(N), -1, -2), In, dtype)


def any_order_bound(K, u, absref):
    """Worst case of a K-term inner product of exactly represented operands, products and sums rounded to unit roundoff u
    in ANY order, pairwise or chained, fused or not: every term passes at most K roundings (its product and at most
    K - 1 additions), so |got - ref| <= ((1 + u)^K - 1) sum |a_q| |x_q| <= 1.01 K u sum |a_q| |x_q| for K u < 0.01.  The
    eight extra roundings cover the 1.01, the additions of partial results that the callers make outside the kernel
    (K slices by atomicAdd, the fp64 sum over at most seven time slices) and the rounding of the fp64 reference itself.
    Derived, not measured."""
    return (K + 8) * u * absref


# ---- data --------------------------------------------------------------------------------------------------------------
def exact_data(rng, shape, dtype=np.float32):
    """integers, uniform in [-7, 7]"""
    return rng.integers(-EXACT_ABS, EXACT_ABS + 1, size=shape).astype(dtype)


def rounded_data(rng, shape, decades=False, dtype=np.float32):
    """standard normals; decades: row i of the last-but-one axis scaled by 10^(3 i / (rows - 1))"""
    a = rng.standard_normal(shape)
    if decades:
        a = a * np.logspace(0, 3, shape[-2])[:, None]
    return a.astype(dtype)


KINDS = ("exact", "rounded")


def make_data(kind, rng, shape, decades=False, dtype=np.float32):
    return exact_data(rng, shape, dtype) if kind == "exact" else rounded_data(rng, shape, decades, dtype)


# ---- tile_atx cases ----------------------------------------------------------------------------------------------------
# entry: the C entry point; ld: "time" = pmd_time_ld(T), "r32" = round_up(T, 32); form: "pix" (pixel lists with
# pix_stride = d + 3, the spare ids naming a guard row of NaN), "tight" (pix_stride = d), "row0" (pix NULL, row0_stride
# d + 1), "shared_a" (a_tile_stride 0); rows: hint (0: none); ranks: per-tile ranks or None; kinds: data kinds to run
AtxCase = namedtuple("AtxCase", "entry d T slices ld env n_tiles form rows ranks kinds")

ATX_D = (1, 15, 16, 17, 255, 256, 257, 399, 400, 401, 512, 513, 799, 800, 801, 1023, 1024, 1025, 2048, 2049, 2500)
ATX_T = (1, 31, 32, 33, 64, 65, 97, 129, 161)
ATX_SLICES = (1, 2, 3, 100)
ATX_TMAX = max(ATX_T)
ATX_ROWS_D = (513, 800, 1000, 1024)
ATX_ROWS = (1, 16, 17)
ATX_RANKED_D = (257, 400)
ATX_RANKS = (0, 1, 32, 33, 64)
ATX_SUB_T = (1, 33, 97, 161)
ATX_PROJECT_D = (17, 257, 400, 513, 1024, 1025)
ATX_COUNTS = (64, 67, 71, 130)
ATX_COUNT_SHAPES = ((48, 70, 3), (1100, 40, 2))     # (d, T, slices)


def atx_ldx(case):
    return time_ld(case.T) if case.ld == "time" else round_up(case.T, 32)


def atx_route(case, rank=None):
    return route_of_atx(case.d, case.T, atx_ldx(case), switch(case.env, "PMD_ATX_DMA", 1), case.rows, rank)


def atx_shape_cases(d):
    """pmdk_tile_atx at one d: every T and slice count on every route of that d, then the argument forms"""
    routes = [("default", "time")]
    if 256 < d <= 400:
        routes += [("default", "r32"), ("atx_dma0", "time")]
    out = [AtxCase("pmdk_tile_atx", d, T, s, ld, env, 3, "pix", 0, None, KINDS) for env, ld in routes for T in ATX_T for s in ATX_SLICES]
    if not 256 < d <= 400:
        out += [AtxCase("pmdk_tile_atx", d, T, 2, "r32", "default", 3, "pix", 0, None, KINDS) for T in ATX_T]
    out += [AtxCase("pmdk_tile_atx", d, T, 2, "time", "default", 3, form, 0, None, KINDS) for form in ("row0", "shared_a") for T in ATX_T]
    return out


def atx_rows_cases(d):
    return [AtxCase("pmdk_tile_atx_rows", d, T, s, "time", "default", 3, "pix", rows, None, KINDS)
            for rows in ATX_ROWS for T in ATX_SUB_T for s in (1, 3)]


def atx_ranked_cases(d):
    return [AtxCase("pmd_tiles_project_ranked", d, T, s, ld, env, len(ATX_RANKS), "tight", 0, ATX_RANKS, KINDS)
            for env, ld in (("default", "time"), ("default", "r32"), ("atx_dma0", "time")) for T in ATX_SUB_T for s in (1, 2, 3)]


def atx_project_cases(d):
    return [AtxCase("pmd_tiles_project", d, T, 2, "time", "default", 3, "tight", 0, None, KINDS) for T in (33, 161)]


def atx_count_cases(shape):
    d, T, s = shape
    return [AtxCase("pmdk_tile_atx", d, T, s, "time", "default", n, "pix", 0, None, ("exact",)) for n in ATX_COUNTS]


def atx_cases():
    out = []
    for d in ATX_D:
        out += atx_shape_cases(d)
    for d in ATX_ROWS_D:
        out += atx_rows_cases(d)
    for d in ATX_RANKED_D:
        out += atx_ranked_cases(d)
    for d in ATX_PROJECT_D:
        out += atx_project_cases(d)
    for shape in ATX_COUNT_SHAPES:
        out += atx_count_cases(shape)
    return out


# ---- tile_xbt cases ----------------------------------------------------------------------------------------------------
# form: "pix" (pix_stride d + 3, guard row), "row0" (pix NULL, row0_stride d + 1), "shared_b" (b_tile_stride 0),
# "stride0" (slices 1 with s_slice_stride 0, as the drivers call it)
XbtCase = namedtuple("XbtCase", "d T slices n_tiles form kinds")

XBT_D = (1, 17, 64, 65, 128, 129, 256, 257, 448, 449, 1024)
XBT_T = (1, 15, 16, 17, 33, 48, 80, 133, 144, 1000)
XBT_SLICES = (4, 1, 3)
XBT_MANY = XbtCase(65, 33, 4, 67, "pix", ("exact",))


def xbt_shape_cases(d):
    out = [XbtCase(d, T, s, 3, "pix", KINDS) for T in XBT_T for s in XBT_SLICES]
    out += [XbtCase(d, T, 4, 3, form, KINDS) for form in ("row0", "shared_b") for T in (17, 133)]
    out += [XbtCase(d, T, 1, 3, "stride0", KINDS) for T in (17, 133)]
    return out


def xbt_cases():
    out = [XBT_MANY]
    for d in XBT_D:
        out += xbt_shape_cases(d)
    return out


# ---- tile_gram cases ---------------------------------------------------------------------------------------------------
# offset: floats the base pointer is moved by (1: rows not 16-byte aligned)
GramCase = namedtuple("GramCase", "len slices ld env offset n_tiles kinds")

GRAM_LEN = (1, 3, 31, 32, 33, 100, 1234)
GRAM_SLICES = (1, 2, 4, 7)


def gram_route(case):
    return route_of_gram(case.ld, 64 * case.ld, case.offset % 4 == 0, switch(case.env, "PMD_GRAM_MFMA", 1))


def gram_len_cases(length):
    out = []
    for s in GRAM_SLICES:
        for ld in sorted({time_ld(length), round_up(length, 4), length}):
            out += [GramCase(length, s, ld, env, 0, 3, KINDS) for env in ("default", "gram0")]
        out.append(GramCase(length, s, time_ld(length), "default", 1, 3, KINDS))
    return out


def gram_cases():
    out = []
    for length in GRAM_LEN:
        out += gram_len_cases(length)
    return out


# ---- tile_rowmix cases -------------------------------------------------------------------------------------------------
# n_stride: n_tile_stride (4096: one matrix per tile; 0: shared; 1: overlapping windows of one buffer, every tile its own)
RowmixCase = namedtuple("RowmixCase", "n_in n_out len ld_in ld_out inplace n_stride env n_tiles kinds")

ROWMIX_SHAPES = ((1, 1), (3, 4), (50, 5), (50, 37), (64, 64), (64, 33), (17, 32))
ROWMIX_LEN = (1, 3, 4, 15, 16, 17, 63, 64, 65, 1100)
ROWMIX_ENVS = ("default", "rowmix0", "rowmix16", "rowmix64")
ROWMIX_MANY = (RowmixCase(50, 37, 8, 8, 8, True, 1, "default", 8191, ("exact",)),
               RowmixCase(50, 37, 8, 8, 8, True, 1, "default", 8192, ("exact",)),
               RowmixCase(50, 37, 4, 4, 4, False, 1, "default", 32769, ("exact",)))


def rowmix_route(case):
    return route_of_rowmix(case.n_out, case.len, case.ld_in, case.ld_out, 64 * case.ld_in, 64 * case.ld_out, case.n_tiles,
                           rowmix_mfma=switch(case.env, "PMD_ROWMIX_MFMA", -1))


def rowmix_env_cases(env):
    out = []
    for i, (n_in, n_out) in enumerate(ROWMIX_SHAPES):
        for j, length in enumerate(ROWMIX_LEN):
            ld = round_up(length, 4) + 4
            n_stride = 4096 if (i + j) % 2 == 0 else 0
            out.append(RowmixCase(n_in, n_out, length, ld, ld, True, n_stride, env, 3, KINDS))
            out.append(RowmixCase(n_in, n_out, length, ld, ld + 4, False, 4096 - n_stride, env, 3, KINDS))
        # rows that are not 16-byte aligned, and rows without a spare position
        for length in (3, 17, 65):
            out.append(RowmixCase(n_in, n_out, length, round_up(length, 4) + 1, round_up(length, 4) + 1, True, 4096, env, 3, KINDS))
            out.append(RowmixCase(n_in, n_out, length, length, length + 3, False, 0, env, 3, KINDS))
    return out


def rowmix_cases():
    out = list(ROWMIX_MANY)
    for env in ROWMIX_ENVS:
        out += rowmix_env_cases(env)
    return out


# ---- the largest integer an exact case can reach -----------------------------------------------------------------------
def exact_magnitude(case):
    """upper limit of |any partial sum| of an exact case: 49 per term"""
    terms = {AtxCase: lambda c: c.d, XbtCase: lambda c: round_up(c.T, 16), GramCase: lambda c: c.len,
             RowmixCase: lambda c: c.n_in}[type(case)](case)
    return EXACT_ABS * EXACT_ABS * terms
