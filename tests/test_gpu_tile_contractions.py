"""
The four 64-row tile contractions of csrc/tile_gemm.hip, kernel by kernel (GPU): pmdk_tile_atx (with pmdk_tile_atx_rows,
pmd_tiles_project and pmd_tiles_project_ranked), pmdk_tile_xbt, pmdk_tile_gram and pmdk_tile_rowmix on every route their
launchers can choose, against float64.  tests/tile_gemm_ref.py holds the cases, the references and the restated launch
decisions; tests/test_tile_gemm_ref.py proves, without a GPU, that the cases reach every kernel instantiation.

Every case runs on two kinds of data:
  exact    integer operands in [-7, 7]: every partial sum in any order is an integer below 2^24, so the result must equal
           the reference bit for bit - a dropped, doubled or misplaced term, stale staging data or a wrong tile shows
           whatever the summation order;
  rounded  normal operands: every entry on its own within the worst case of a sum in any order,
           |got - ref| <= (K + 8) u sum |a_q| |x_q|   (tile_gemm_ref.any_order_bound: derived, not measured).
Whatever a kernel writes is pre-filled with a NaN of a payload no arithmetic produces, so "not written" is checked to the
bit; whatever a kernel may read without using it holds NaN.
"""
import numpy as np
import pytest

from tests import tile_gemm_ref as R
from tests.util import context_under

pytestmark = pytest.mark.gpu

PRE32 = 0x7FC12345
PRE64 = 0x7FF8000012345678
SENTINEL = 4097.5              # finite, nonzero, no value an exact case can produce

# largest observed error / bound per family, over the rounded cases (printed by the last test; for information)
WORST = {"tile_atx": 0.0, "tile_xbt": 0.0, "tile_gram": 0.0, "tile_rowmix": 0.0}


def _t():
    import torch

    return torch


def P(t):
    from localmd_amd._lib import ptr

    return ptr(t)


def dev(ctx, a):
    return _t().from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def prefilled(ctx, shape, double=False):
    torch = _t()
    if double:
        return torch.full(shape, PRE64, dtype=torch.int64, device=ctx.device).view(torch.float64)
    return torch.full(shape, PRE32, dtype=torch.int32, device=ctx.device).view(torch.float32)


def kept(a):
    """where the prefill is still there, to the bit"""
    return a.view(np.int64) == PRE64 if a.dtype == np.float64 else a.view(np.int32) == PRE32


def same_bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.fixture(scope="module")
def ctxs(gpu_ctx):
    """name of tile_gemm_ref.ENVS -> context with those route switches; made on first use, closed with the module"""
    made = {"default": gpu_ctx}

    def get(name):
        if name not in made:
            made[name] = context_under(R.ENVS[name])
        return made[name]

    yield get
    for name, ctx in made.items():
        if name != "default":
            ctx.close()


def check(family, kind, got, ref, absref, K, u, what, extra=0.0):
    """exact: bit for bit (no margin); rounded: entry by entry within the any-order bound"""
    got = got.astype(ref.dtype)
    if kind == "exact":
        bad = got != ref
        assert not bad.any(), (what, "exact", int(bad.sum()), np.argwhere(bad)[:4].tolist())
        return
    bound = R.any_order_bound(K, u, absref) + extra
    err = np.abs(got - ref)
    ok = err <= bound
    assert ok.all(), (what, "rounded", int((~ok).sum()), np.argwhere(~ok)[:4].tolist(),
                      float(np.nanmax(err / np.maximum(bound, 1e-300))))
    if (bound > 0).any():
        WORST[family] = max(WORST[family], float((err[bound > 0] / bound[bound > 0]).max()))


# ---- tile_atx ------------------------------------------------------------------------------------------------------
class AtxData:
    """Operands of n tiles of d pixels over t_max frames and their reference; device copies are made per context."""

    def __init__(self, kind, d, n_tiles, form, t_max, seed, rows=0, ranks=None):
        rng = np.random.default_rng(seed)
        self.kind, self.d, self.n, self.form, self.t_max = kind, d, n_tiles, form, t_max
        self.dpad = R.tile_dpad(d)
        self.row0 = d + 1
        n_rows = n_tiles * self.row0 + 1 if form == "row0" else d + 72
        guard = n_rows - 1
        self.X = R.make_data(kind, rng, (n_rows, t_max))
        self.X[guard] = np.nan
        if form != "row0":
            self.pix_stride = d if form == "tight" else d + 3
            self.pix = np.full((n_tiles, self.pix_stride), guard, dtype=np.int32)   # spare ids: the in-range guard row
            for t in range(n_tiles):
                self.pix[t, :d] = rng.permutation(guard)[:d]
            rows_of = self.pix[:, :d]
        else:
            self.pix_stride, self.pix = d, None
            rows_of = np.arange(n_tiles)[:, None] * self.row0 + np.arange(d)[None, :]
        n_a = 1 if form == "shared_a" else n_tiles
        self.A = np.zeros((n_a, 64, self.dpad), dtype=np.float32)
        for t in range(n_a):
            top = ranks[t] if ranks is not None else rows if rows else 64
            self.A[t, :top, :d] = R.make_data(kind, rng, (top, d))
        a_ref = np.broadcast_to(self.A, (n_tiles, 64, self.dpad))[:, :, :d]
        self.ref, self.absref = R.ref_atx(a_ref, self.X[rows_of])
        self.ranks = None if ranks is None else np.asarray(ranks, dtype=np.int32)
        self._dev = None

    def on(self, ctx):
        if self._dev is None:
            self._dev = (dev(ctx, self.X), dev(ctx, self.A), None if self.pix is None else dev(ctx, self.pix),
                         None if self.ranks is None else dev(ctx, self.ranks), {})
        return self._dev

    def x_for(self, ctx, T, ldx):
        """X with T frames at leading dimension ldx; every column from T on holds NaN"""
        xfull, _, _, _, cache = self.on(ctx)
        if (T, ldx) not in cache:
            cache.clear()      # one padded copy at a time
            x = _t().full((self.X.shape[0], ldx), float("nan"), dtype=_t().float32, device=ctx.device)
            x[:, :T] = xfull[:, :T]
            cache[(T, ldx)] = x
        return cache[(T, ldx)]


def run_atx(ctx, case, data, entry=None):
    T, d, n = case.T, case.d, data.n
    ldx, ldo = R.atx_ldx(case), R.round_up(T, 32) + 32
    _, a_d, pix_d, ranks_d, _ = data.on(ctx)
    x_d = data.x_for(ctx, T, ldx)
    out = prefilled(ctx, (n, 64, ldo))
    a_stride = 0 if data.form == "shared_a" else 64 * data.dpad
    entry = entry or case.entry
    if entry in ("pmdk_tile_atx", "pmdk_tile_atx_rows"):
        extra = (case.rows,) if entry == "pmdk_tile_atx_rows" else ()
        ctx.call(entry, P(x_d), ldx, P(pix_d), data.pix_stride, data.row0, d, P(a_d), a_stride, data.dpad, P(out), 64 * ldo, ldo,
                 n, T, case.slices, *extra)
    else:
        assert data.form == "tight"
        extra = (P(ranks_d),) if entry == "pmd_tiles_project_ranked" else ()
        ctx.call(entry, P(x_d), ldx, T, P(pix_d), n, d, P(a_d), data.dpad, P(out), ldo, case.slices, *extra)
    ctx.sync()
    return out.cpu().numpy()


def check_atx(case, data, got):
    T, d = case.T, case.d
    r32 = R.round_up(T, 32)
    for t in range(data.n):
        route = R.atx_route(case, None if case.ranks is None else case.ranks[t])
        written = 16 if route == "tile_atx_kernel<8,8,1,1>" else 32 if route.endswith(":half") else 64
        what = (case, t, route)
        check("tile_atx", data.kind, got[t, :written, :T], data.ref[t, :written, :T], data.absref[t, :written, :T], d, R.U32, what)
        assert kept(got[t, written:]).all(), (what, "rows the kernel does not own were written")
        if d <= 1024:
            assert kept(got[t, :, r32:]).all(), (what, "columns behind the last chunk were written")
        else:
            assert np.all(got[t, :, r32:] == 0), (what, "columns behind the last chunk: cleared with the K-split block")


def atx_sweep(ctxs, cases, make, key=lambda case: case.form, repeat=lambda case: False):
    """cases on both kinds of data; make(kind, case) builds the operands of a key once per kind"""
    for kind in R.KINDS:
        store = {}
        for case in cases:
            if kind not in case.kinds:
                continue
            if key(case) not in store:
                store[key(case)] = make(kind, case)
            data = store[key(case)]
            got = run_atx(ctxs(case.env), case, data)
            check_atx(case, data, got)
            if repeat(case):
                assert same_bits(got, run_atx(ctxs(case.env), case, data)), (case, kind, "a second call gave other bits")


@pytest.mark.parametrize("d", R.ATX_D)
def test_tile_atx_shapes(ctxs, d):
    """Every T, slice count and route of one d; pixel lists with spare ids, consecutive rows, one A for all tiles; all 64
    rows of A filled; X holds NaN from frame T on.  Without atomics (d <= 1024) a second call gives the same bits."""
    atx_sweep(ctxs, R.atx_shape_cases(d), lambda kind, case: AtxData(kind, d, 3, case.form, R.ATX_TMAX, seed=1000 + d),
              repeat=lambda c: d <= 1024 and c.slices == 2)


@pytest.mark.parametrize("d", R.ATX_ROWS_D)
def test_tile_atx_row_hint(ctxs, d):
    """pmdk_tile_atx_rows: only `rows` rows of A carry data.  Where the one-row-tile kernel runs (801..1024 pixels, hint <=
    16) rows >= 16 of Out stay untouched; everywhere else the hint changes nothing."""
    atx_sweep(ctxs, R.atx_rows_cases(d), lambda kind, case: AtxData(kind, d, 3, "pix", R.ATX_TMAX, seed=2000 + d, rows=case.rows),
              key=lambda case: case.rows)


@pytest.mark.parametrize("d", R.ATX_RANKED_D)
def test_tiles_project_ranked(ctxs, d):
    """pmd_tiles_project_ranked with ranks 0, 1, 32, 33, 64: on the LDS-DMA route a tile of rank <= 32 runs as a half tile
    and rows >= 32 of its block stay untouched; on the register-staged routes every row is written."""
    atx_sweep(ctxs, R.atx_ranked_cases(d),
              lambda kind, case: AtxData(kind, d, len(R.ATX_RANKS), "tight", R.ATX_TMAX, seed=3000 + d, ranks=R.ATX_RANKS),
              repeat=lambda c: c.slices == 2)


@pytest.mark.parametrize("d", R.ATX_PROJECT_D)
def test_tiles_project_equals_tile_atx(ctxs, d):
    """pmd_tiles_project is pmdk_tile_atx with pix_stride = d and tile strides of 64 rows: same bits (with atomics,
    d > 1024, on the exact data, whose sums have no rounding to reorder), and right."""
    ctx = ctxs("default")
    for kind in R.KINDS:
        data = AtxData(kind, d, 3, "tight", R.ATX_TMAX, seed=4000 + d)
        for case in R.atx_project_cases(d):
            got = run_atx(ctx, case, data)
            check_atx(case, data, got)
            if kind == "exact" or d <= 1024:
                assert same_bits(got, run_atx(ctx, case, data, entry="pmdk_tile_atx")), (case, kind)


@pytest.mark.parametrize("shape", R.ATX_COUNT_SHAPES, ids=lambda s: "d%d" % s[0])
def test_tile_atx_tile_order(ctxs, shape):
    """From 64 tiles on the workgroups are dealt to tiles in XCD order, by grid row and K slice: 64, 67, 71 and 130 pairwise
    different tiles, each of which must come out in its own place."""
    data = {}
    for case in R.atx_count_cases(shape):
        # the first n tiles of one data set of 130
        if not data:
            data["all"] = AtxData("exact", case.d, max(R.ATX_COUNTS), "pix", case.T, seed=5000 + case.d)
            ref = data["all"].ref
            assert len({ref[t].tobytes() for t in range(ref.shape[0])}) == ref.shape[0]
        full = data["all"]
        full.n = case.n_tiles
        got = run_atx(ctxs("default"), case, full)
        check_atx(case, full, got)


# ---- tile_xbt ------------------------------------------------------------------------------------------------------
class XbtData:
    def __init__(self, kind, d, n_tiles, t_max, seed):
        rng = np.random.default_rng(seed)
        self.kind, self.d, self.n = kind, d, n_tiles
        self.row0 = d + 1
        self.n_rows = max(n_tiles * self.row0 + 1, d + 72) if n_tiles <= 3 else d + 72
        self.guard = self.n_rows - 1
        self.t_full = R.round_up(t_max, 16)
        self.X = R.make_data(kind, rng, (self.n_rows, self.t_full))
        self.B = R.make_data(kind, rng, (n_tiles, 64, self.t_full))
        self.pix_stride = d + 3
        self.pix = np.full((n_tiles, self.pix_stride), self.guard, dtype=np.int32)
        for t in range(n_tiles):
            self.pix[t, :d] = rng.permutation(min(self.guard, d + 71))[:d]
        self._dev, self._refs = None, {}

    def on(self, ctx):
        if self._dev is None:
            self._dev = (dev(ctx, self.X), dev(ctx, self.B), dev(ctx, self.pix))
        return self._dev

    def ref(self, form, T):
        """computed once per operand form and T, shared by the slice counts"""
        key = ("row0" if form == "row0" else "shared_b" if form == "shared_b" else "pix", T)
        if key not in self._refs:
            b = self.B[:1] if form == "shared_b" else self.B
            self._refs[key] = R.ref_xbt(np.broadcast_to(b, (self.n, 64, self.t_full))[:, :, :T], self.X[self.rows_of(form)][:, :, :T])
        return self._refs[key]

    def rows_of(self, form):
        if form == "row0":
            return np.arange(self.n)[:, None] * self.row0 + np.arange(self.d)[None, :]
        return self.pix[:, :self.d]


def run_xbt(ctx, case, data):
    """The padding contract of the header: in frames [T, round_up(T, 16)) X is zero and B holds finite garbage (the frames
    that follow in the full data); from round_up(T, 16) on both hold NaN, and so does the guard row."""
    torch = _t()
    T, d, n = case.T, case.d, data.n
    r16, ldx = R.round_up(T, 16), R.time_ld(T)
    ldb = ldx + 16
    xfull, bfull, pix_d = data.on(ctx)
    x = torch.full((data.n_rows, ldx), float("nan"), dtype=torch.float32, device=ctx.device)
    x[:, :T] = xfull[:, :T]
    x[:, T:r16] = 0
    x[data.guard] = float("nan")
    n_b = 1 if case.form == "shared_b" else n
    b = torch.full((n_b, 64, ldb), float("nan"), dtype=torch.float32, device=ctx.device)
    b[:, :, :r16] = bfull[:n_b, :, :r16]
    mt16 = 16 * R.ceil_div(d, 16)
    s_ld = mt16 + 16
    S = prefilled(ctx, (n, case.slices, 64, s_ld))
    slice_stride = 0 if case.form == "stride0" else 64 * s_ld
    ctx.call("pmdk_tile_xbt", P(x), ldx, P(None if case.form == "row0" else pix_d), data.pix_stride, data.row0, d, P(b),
             0 if case.form == "shared_b" else 64 * ldb, ldb, P(S), case.slices * 64 * s_ld, slice_stride, s_ld, n, T, case.slices)
    ctx.sync()
    return S.cpu().numpy()


def check_xbt(case, data, S):
    T, d, n = case.T, case.d, data.n
    mt16 = 16 * R.ceil_div(d, 16)
    _, work, _, _ = R.xbt_launch(d, T, case.slices)
    assert np.isfinite(S[:, :, :, :mt16]).all(), (case, "a slice the caller asked for is not finite")
    assert np.all(S[:, work:] == 0), (case, "slices without work must be cleared")
    assert np.all(S[:, :work, :, d:mt16] == 0), (case, "pixels behind the tile's last one")
    assert kept(S[:, :work, :, mt16:]).all(), (case, "columns behind the last pixel tile were written")
    ref, absref = data.ref(case.form, T)
    total = S[:, :, :, :d].astype(np.float64).sum(axis=1)
    check("tile_xbt", data.kind, total, ref, absref, R.round_up(T, 16), R.U32, case)


@pytest.mark.parametrize("d", R.XBT_D)
def test_tile_xbt_shapes(ctxs, d):
    """Every T on 4, 1 and 3 slices; pixel lists with spare ids, consecutive rows, one B for all tiles, the one-slice form
    with s_slice_stride 0.  No atomics: a second call gives the same bits."""
    ctx = ctxs("default")
    for kind in R.KINDS:
        data = XbtData(kind, d, 3, max(R.XBT_T), seed=6000 + d)
        for case in R.xbt_shape_cases(d):
            S = run_xbt(ctx, case, data)
            check_xbt(case, data, S)
            if case.slices == 3:
                assert same_bits(S, run_xbt(ctx, case, data)), (case, kind, "a second call gave other bits")


def test_tile_xbt_many_tiles(ctxs):
    """67 pairwise different tiles (XCD order), three frame groups for four slices: the fourth is cleared for every tile"""
    case = R.XBT_MANY
    data = XbtData("exact", case.d, case.n_tiles, case.T, seed=6500)
    check_xbt(case, data, run_xbt(ctxs("default"), case, data))


# ---- tile_gram -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", R.GRAM_LEN)
def test_tile_gram(ctxs, length):
    """MFMA and scalar kernel, the latter by switch, by leading dimension and by alignment; NaN in every position >= len;
    every slice finite, slices without positions zero, the slice sum right and symmetric to the bit."""
    torch = _t()
    for kind in R.KINDS:
        rng = np.random.default_rng(7000 + length)
        data = R.make_data(kind, rng, (3, 64, length), decades=True)
        ref, absref = R.ref_gram(data, np.float64 if kind == "exact" else np.longdouble)
        for case in R.gram_len_cases(length):
            ctx = ctxs(case.env)
            ld = case.ld
            buf = torch.full((3 * 64 * ld + case.offset,), float("nan"), dtype=torch.float32, device=ctx.device)
            inp = buf[case.offset:].view(3, 64, ld)
            inp[:, :, :length] = dev(ctx, data)
            runs = []
            for _ in range(2 if case.slices == 2 else 1):
                G = prefilled(ctx, (3, case.slices, 64, 64), double=True)
                ctx.call("pmdk_tile_gram", P(inp), 64 * ld, ld, length, 3, case.slices, P(G))
                ctx.sync()
                runs.append(G.cpu().numpy())
            g = runs[0]
            assert np.array_equal(g.view(np.int64), runs[-1].view(np.int64)), (case, "a second call gave other bits")
            what = (case, R.gram_route(case))
            assert np.isfinite(g).all(), (what, "a slice is not finite")
            first_empty = R.ceil_div(length, R.gram_chunk(length, case.slices))
            assert np.all(g[:, first_empty:] == 0), (what, "slices without positions must be zero")
            total = g.sum(axis=1)
            check("tile_gram", kind, total, ref, absref, length, R.U64, what)
            assert np.array_equal(total, np.swapaxes(total, 1, 2)), (what, "not symmetric to the bit")


# ---- tile_rowmix ---------------------------------------------------------------------------------------------------
def run_rowmix(ctx, case, kind, rng):
    """Rows >= n_in of In and entries of N outside n_in x n_out hold NaN.  Positions from len on: NaN out of place (the
    kernels may read, not use, them); in place a finite sentinel, so that a write there shows."""
    torch = _t()
    n, n_in, n_out, length = case.n_tiles, case.n_in, case.n_out, case.len
    data = R.make_data(kind, rng, (n, n_in, length), decades=True)
    host_in = np.full((n, 64, case.ld_in), SENTINEL if case.inplace else np.nan, dtype=np.float32)
    host_in[:, :, :length] = np.nan
    host_in[:, :n_in, :length] = data
    if case.n_stride == 1:
        nbuf = R.make_data(kind, rng, (4096 + n,), dtype=np.float64)
        n_d, mats = dev(ctx, nbuf), None
    else:
        n_mats = n if case.n_stride else 1
        mats = R.make_data(kind, rng, (n_mats, n_in, n_out), dtype=np.float64)
        host_n = np.full((n_mats, 64, 64), np.nan)
        host_n[:, :n_in, :n_out] = mats
        n_d = dev(ctx, host_n)
    in_d = dev(ctx, host_in)
    out_d = in_d if case.inplace else prefilled(ctx, (n, 64, case.ld_out))
    ctx.call("pmdk_tile_rowmix", P(in_d), 64 * case.ld_in, case.ld_in, P(n_d), case.n_stride, n_in, n_out, P(out_d), 64 * case.ld_out,
             case.ld_out, length, n)
    ctx.sync()
    out = out_d.cpu().numpy()
    what = (case, R.rowmix_route(case))
    if case.inplace:
        assert same_bits(out[:, :, length:], host_in[:, :, length:]), (what, "written from len on")
    else:
        assert kept(out[:, :, length:]).all(), (what, "written from len on")
        assert same_bits(in_d.cpu().numpy(), host_in), (what, "the input changed")
        if n <= 3:
            again = prefilled(ctx, (n, 64, case.ld_out))
            ctx.call("pmdk_tile_rowmix", P(in_d), 64 * case.ld_in, case.ld_in, P(n_d), case.n_stride, n_in, n_out, P(again), 64 * case.ld_out,
                     case.ld_out, length, n)
            ctx.sync()
            assert same_bits(out, again.cpu().numpy()), (what, "a second call gave other bits")
    assert np.all(out[:, n_out:, :length] == 0), (what, "rows [n_out, 64) must be zero up to len")
    dtype = np.float64 if kind == "exact" else np.longdouble
    if mats is not None:
        ref, absref = R.ref_rowmix(np.broadcast_to(mats, (n, n_in, n_out)), data, dtype)
        check("tile_rowmix", kind, out[:, :n_out, :length], ref, absref, n_in, R.U64, what, extra=R.U32 * np.abs(ref))
        return
    # tile t mixes with the 64 x 64 window that starts at element t of one buffer: every tile its own matrix
    windows = np.lib.stride_tricks.sliding_window_view(nbuf, 4096)
    for t0 in range(0, n, 1024):
        t1 = min(n, t0 + 1024)
        mats = windows[t0:t1].reshape(t1 - t0, 64, 64)[:, :n_in, :n_out]
        ref, absref = R.ref_rowmix(mats, data[t0:t1], dtype)
        check("tile_rowmix", kind, out[t0:t1, :n_out, :length], ref, absref, n_in, R.U64, (what, t0), extra=R.U32 * np.abs(ref))


@pytest.mark.parametrize("env", R.ROWMIX_ENVS)
def test_tile_rowmix(ctxs, env):
    """All five kernels by shape and by PMD_ROWMIX_MFMA: in place and out of place, one matrix per tile and a shared one,
    ld_out != ld_in, rows that are not 16-byte aligned and rows without a spare position (where the 64-position form gives
    way to the 16-position one)."""
    for kind in R.KINDS:
        rng = np.random.default_rng(8000)
        for case in R.rowmix_env_cases(env):
            run_rowmix(ctxs(env), case, kind, rng)


@pytest.mark.parametrize("case", R.ROWMIX_MANY, ids=lambda c: "tiles%d" % c.n_tiles)
def test_tile_rowmix_many_tiles(ctxs, case):
    """The switch to the 64-position form at 8192 tiles and the second pass of the 32768-tile loop, every tile with its own
    input and its own mixing matrix."""
    run_rowmix(ctxs(case.env), case, "exact", np.random.default_rng(9000 + case.n_tiles))


def test_zz_report_worst_ratios():
    """For information: the largest error / bound each family showed on the rounded data (pytest -s prints it)."""
    print("\nlargest observed error / derived bound:", {k: "%.3g" % v for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())
