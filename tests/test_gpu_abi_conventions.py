"""
The conventions at the top of include/pmd_hip.h, tested as such (the kernel-by-kernel modules test outputs): a workspace of
exactly the reported size is enough and its contents do not matter; a too-small one is refused before anything is launched;
all work is enqueued on the context's stream; contexts are independent and their scratch can be trimmed.  The rows are in
tests/abi_cases.py.

1. Exact size, guard bands, contents.  [front guard 64 KiB | workspace of exactly the reported bytes, 256-byte aligned | back
   guard >= the workspace and >= 64 KiB] in one uint8 tensor; the call on 0xFF, on 0x00 and on twice the size: return code 0,
   both guards unchanged byte for byte, outputs bit-identical (after two calls on the same fill were).
2. Refusals.  NULL / 0 and half the bytes (wherever the size function's slack, abi_cases.SLACK, cannot cover the other half,
   and always from 1 MiB on: every mandatory row but gram_mtgm-131x1, which reports 4864 bytes of which 4096 are slack) return
   PMD_ERR_WORKSPACE with outputs, inputs, guards and the workspace itself unchanged and a pmd_last_error text; the next
   sized call on the same context returns the bits of 1.  reported - 1 bytes may be refused or give those bits.
3. Host restatements of the size functions against the library (no GPU needed, only the built library).
4. Streams.  A context made under a non-blocking side stream; the inputs hold a valid set B; on the side stream: a delay, an
   event, copies of set A into the inputs, the call.  Whatever part of the call ran on another stream started while the
   inputs held B, so the result must be the bits of the call on A on the session context (null stream).  The event must
   still be pending after the copies are enqueued, else the case fails as inconclusive.  pmd_threshold_sim has no device
   input: there the check is that nothing has written its output while the delay still runs.
   Measured on an MI355X: the delay (torch.cuda._sleep, sized by a calibration run to DELAY_MS = 150: 359 727 402 ticks) took
   149.9 ms; enqueuing it and its event took 0.012 - 0.038 ms and enqueuing the copies 0.001 - 0.016 ms over all cases of
   three runs, so the event is queried some 0.05 ms into a 150 ms delay.
5. Two contexts at once as the driver's Cholesky step runs them, pmd_scratch_trim, a fresh against the warmed context.
"""
import re
import time

import pytest

from tests import abi_cases as T
from tests.abi_cases import PMD_ERR_WORKSPACE, same_bits
from tests.util import context_under

gpu = pytest.mark.gpu

GUARD = 64 << 10
DELAY_MS = 150.0
F16_ENV = {"PMD_GEMM_SPLIT_MIN_GFLOP": "0", "PMD_GEMM_SPLIT_MIN_DIM": "1"}
OWN_SYEVD_ENV = {"PMD_SYEVD": "own"}


def _t():
    import torch

    return torch


@pytest.fixture(scope="module")
def cases(gpu_ctx):
    """row name -> Case, built on first use and kept for the module (the rows are small)."""
    built = {}

    def get(row):
        if row not in built:
            built[row] = T.ALL[row](gpu_ctx)
        return built[row]

    yield get
    built.clear()


class Guarded:
    """[front guard | workspace of n bytes on a 256-byte boundary | back guard], every byte = fill."""

    def __init__(self, ctx, n, fill):
        torch = _t()
        self.n, self.fill = int(n), fill
        back = max(self.n, GUARD)
        self.buf = torch.empty(GUARD + 256 + self.n + back, dtype=torch.uint8, device=ctx.device)
        self.buf.fill_(fill)
        self.off = GUARD + (-(self.buf.data_ptr() + GUARD)) % 256
        self.ptr = self.buf.data_ptr() + self.off
        assert self.ptr % 256 == 0 and self.buf.numel() - self.off - self.n >= back

    def guards_intact(self, used=None):
        """Every byte outside [off, off + used) still holds the fill (used: the ws_bytes the call was given)."""
        used = self.n if used is None else used
        return bool((self.buf[:self.off] == self.fill).all()) and bool((self.buf[self.off + used:] == self.fill).all())


def run_guarded(ctx, case, fill=0xFF, factor=1, given=None):
    """The call on inputs A with a guarded workspace of factor x the reported bytes (given: the ws_bytes passed instead).
    On torch's current stream, which must be the context's.  Returns (return code, bits, guards intact, the Guarded)."""
    case.load("A")
    g = Guarded(ctx, case.nbytes * factor, fill)
    used = g.n if given is None else given
    rc = case.run(ctx, g.ptr if used else None, used)
    _t().cuda.current_stream().synchronize()
    return rc, case.bits(), g.guards_intact(used), g


def reference(ctx, case):
    """Bits of the call on inputs A on the session context, exactly sized workspace full of 0xFF."""
    if case.reference is None:
        rc, bits, ok, _ = run_guarded(ctx, case)
        assert rc == 0 and ok
        case.reference = bits
    return case.reference


# =====================================================================================================================
# 0. the table
def test_table_lists_every_size_function():
    """Every *_workspace_bytes / *_work_floats function of the header has a row or a pointer to the test that covers it."""
    import os

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pmd_hip.h")).read()
    declared = set(re.findall(r"^(?:size_t|long)\s+(pmdk?_\w+_(?:workspace_bytes|work_floats))\(", header, flags=re.M))
    rows = {T.size_function_of(r) for r in list(T.MANDATORY) + list(T.CONSUMERS)}
    assert len(declared) >= 26, sorted(declared)
    assert not rows & set(T.COVERED_ELSEWHERE)
    assert declared == rows | set(T.COVERED_ELSEWHERE), (sorted(declared - rows - set(T.COVERED_ELSEWHERE)),
                                                         sorted((rows | set(T.COVERED_ELSEWHERE)) - declared))


# =====================================================================================================================
# 1. exact size, guard bands, contents
@gpu
@pytest.mark.parametrize("row", list(T.MANDATORY) + list(T.CONSUMERS))
def test_exact_workspace_guard_bands_and_contents(gpu_ctx, cases, row):
    case = cases(row)
    assert case.nbytes > 0
    runs = {}
    for label, fill, factor in (("0xFF", 0xFF, 1), ("0xFF again", 0xFF, 1), ("0x00", 0x00, 1), ("0xFF, twice the size", 0xFF, 2)):
        rc, bits, intact, _ = run_guarded(gpu_ctx, case, fill, factor)
        assert rc == 0, (row, label, rc, gpu_ctx.lib.pmd_last_error(gpu_ctx.handle))
        assert intact, (row, label, "a guard band was written")
        runs[label] = bits
    assert same_bits(runs["0xFF"], runs["0xFF again"]), (row, "not reproducible call to call on the same workspace fill")
    assert same_bits(runs["0xFF"], runs["0x00"]), (row, "the result depends on the workspace's contents")
    assert same_bits(runs["0xFF"], runs["0xFF, twice the size"]), (row, "the result depends on the workspace's size")
    case.reference = runs["0xFF"]


@gpu
def test_exact_workspace_on_the_rocblas_cholesky_chain(cases):
    """The same on the blocked Cholesky factorisation under PMD_CHOL_CHAIN=rocblas, whose panel product (a plain sgemm) reads
    all of the 128 x 128 inverse block in the workspace, not only the triangle that is the inverse; the default chain masks
    the other triangle in its panel kernel.  (Measured on an MI355X: rocBLAS' strtri clears that triangle itself, so the
    bits are the same with and without the hipMemsetAsync of the block in chol_lower_rm, on both chains.)"""
    case = cases("chol_inverse-641-abs0")
    ctx = context_under({"PMD_CHOL_CHAIN": "rocblas"})
    try:
        runs = []
        for fill, factor in ((0xFF, 1), (0xFF, 1), (0x00, 1), (0xFF, 2)):
            rc, bits, intact, _ = run_guarded(ctx, case, fill, factor)
            assert rc == 0 and intact and bits[-1] == 1, (fill, factor, rc, intact, bits[-1])
            runs.append(bits)
        assert same_bits(runs[0], runs[1]), "not reproducible call to call"
        assert same_bits(runs[0], runs[2]) and same_bits(runs[0], runs[3]), "the result depends on the workspace's contents or size"
    finally:
        ctx.close()


# =====================================================================================================================
# 2. too-small workspaces are refused before anything is launched
@gpu
@pytest.mark.parametrize("row", list(T.MANDATORY))
def test_too_small_workspace_is_refused_untouched(gpu_ctx, cases, row):
    ctx, case = gpu_ctx, cases(row)
    ref = reference(ctx, case)
    refusals = [("NULL, 0", 0)] + ([("half", case.nbytes // 2)] if T.half_is_too_small(case) else [])
    for label, given in refusals:
        rc, _, intact, g = run_guarded(ctx, case, 0xFF, given=given)
        assert rc == PMD_ERR_WORKSPACE, (row, label, rc)
        assert case.untouched("A"), (row, label, "a refused call changed its outputs or inputs")
        assert intact and bool((g.buf == 0xFF).all()), (row, label, "a refused call wrote to the workspace or its guards")
        assert b"workspace" in ctx.lib.pmd_last_error(ctx.handle), (row, label, ctx.lib.pmd_last_error(ctx.handle))
        rc, bits, intact, _ = run_guarded(ctx, case)
        assert rc == 0 and intact and same_bits(bits, ref), (row, label, "the call after a refusal differs")
    rc, bits, intact, _ = run_guarded(ctx, case, 0xFF, given=case.nbytes - 1)
    assert intact, (row, "reported - 1")
    if rc == 0:
        assert same_bits(bits, ref), (row, "reported - 1 bytes were accepted and gave other bits")
    else:
        assert rc == PMD_ERR_WORKSPACE and case.untouched("A"), (row, "reported - 1", rc)
        rc, bits, intact, _ = run_guarded(ctx, case)
        assert rc == 0 and intact and same_bits(bits, ref), (row, "the call after the refusal of reported - 1 differs")


@gpu
def test_stats_stream_finish_refuses_on_its_own(gpu_ctx, cases):
    """The stats_stream row runs accumulate and finish in one go, so its refusals come from accumulate.  Here accumulate has
    a full workspace and only pmd_stats_stream_finish gets none, or half: refused with mean and std untouched, and the
    finish on the full workspace afterwards gives the row's bits."""
    ctx, lib, case = gpu_ctx, gpu_ctx.lib, cases("stats_stream")
    ref = reference(ctx, case)
    mov, (mean, std) = case.ins[0], case.outs
    Tn, D = mov.shape
    case.load("A")
    g = Guarded(ctx, case.nbytes, 0xFF)
    assert lib.pmd_stats_stream_accumulate(ctx.handle, mov.data_ptr(), 0, 0, Tn, Tn, D, 1, g.ptr, g.n) == 0
    ctx.sync()
    held = g.buf.clone()
    for ptr, given in ((None, 0), (g.ptr, (Tn + 1023) // 1024 * D * 12 // 2)):
        assert lib.pmd_stats_stream_finish(ctx.handle, Tn, D, 1, mean.data_ptr(), std.data_ptr(), ptr, given) == PMD_ERR_WORKSPACE
        ctx.sync()
        assert case.untouched("A") and _t().equal(g.buf, held) and b"workspace" in lib.pmd_last_error(ctx.handle)
    assert lib.pmd_stats_stream_finish(ctx.handle, Tn, D, 1, mean.data_ptr(), std.data_ptr(), g.ptr, g.n) == 0
    ctx.sync()
    assert g.guards_intact() and same_bits(case.bits(), ref)


@gpu
def test_orthogonalize_chol_refuses_what_its_second_half_would(gpu_ctx):
    """pmd_orthogonalize_chol carves one workspace twice (pmd_gram_mtgm, then pmd_chol_inverse).  At m = 130 on 131 rows the
    first half needs 70 KB and the second 270 KB (the fp64 copy): a workspace between the two is refused with nothing
    launched, not after M^T G M has been written into Et_out."""
    ctx = gpu_ctx
    case = T.orthogonalize_chol(131, 130)(ctx)
    lib = ctx.lib
    first, second = int(lib.pmd_gram_mtgm_workspace_bytes(131, 130)), int(lib.pmd_chol_inverse_workspace_bytes(130))
    assert first < second <= case.nbytes
    rc, _, intact, g = run_guarded(ctx, case, 0xFF, given=(first + second) // 2)
    assert rc == PMD_ERR_WORKSPACE and case.untouched("A") and intact and bool((g.buf == 0xFF).all())
    rc, bits, intact, _ = run_guarded(ctx, case)
    assert rc == 0 and intact and bits[-1] == 1


# =====================================================================================================================
# 3. host restatements of the size functions
def _lib():
    from localmd_amd import _lib

    return _lib.load()


def test_correlate_workspace_matches_library():
    from localmd_amd import register as RG

    lib = _lib()
    geoms = [(48, 56, 4, 4), (8 + 2, 8 + 2, 1, 1), (33 + 14, 65 + 6, 7, 3), (512, 512, 15, 15), (97, 1031, 31, 1), (4096, 4096, 31, 31)]
    for d1, d2, my, mx in geoms:
        per = int(lib.pmd_shift_correlate_workspace_bytes(1, d1, d2, my, mx))
        assert per > 0
        cap = (64 << 20) // per                  # the launch-group cap: 64 MB worth of frames
        for n in {0, 1, 2, 3, 1024, max(cap - 1, 1), max(cap, 1), cap + 1, 10 ** 6}:
            assert RG.correlate_workspace_bytes(n, d1, d2, my, mx) == lib.pmd_shift_correlate_workspace_bytes(n, d1, d2, my, mx), \
                (n, d1, d2, my, mx)


def test_patch_workspace_matches_library():
    from localmd_amd import piecewise as PW

    lib = _lib()
    grids = [PW.PatchGrid(64, 80, (4, 4), (2, 2), (16, 16), (8, 8)), PW.PatchGrid(30, 31, (1, 2), (1, 1), (8, 9), (8, 9)),
             PW.PatchGrid(512, 512, (15, 15), (3, 3), (128, 128), (86, 86)), PW.PatchGrid(101, 203, (5, 9), (7, 1), (33, 65), (11, 64)),
             PW.PatchGrid(2048, 2048, (31, 31), (7, 7), (64, 64), (32, 32))]
    for pg in grids:
        geom = (pg.d1, pg.d2, *pg.max_shift, *pg.max_deviation, *pg.patch, pg.gy, pg.gx)
        per = int(lib.pmd_patch_correlate_workspace_bytes(1, *geom))
        assert per > 0
        cap = (64 << 20) // per
        for n in {0, 1, 2, 1024, max(cap - 1, 1), max(cap, 1), cap + 1, 10 ** 6}:
            assert PW.patch_workspace_bytes(n, pg) == lib.pmd_patch_correlate_workspace_bytes(n, *geom), (n, geom)


def test_deconvolve_workspace_matches_library():
    import importlib

    DX = importlib.import_module("localmd_amd.deconvolve")     # (the package's attribute of that name is the function)
    lib = _lib()
    for Tn in (0, 1, 2, 999, 10 ** 6):
        for n_prob in (0, 1, 63, 64, 65, 10 ** 5):
            assert DX.workspace_bytes(Tn, n_prob) == lib.pmd_oasis_ar1_workspace_bytes(Tn, n_prob), (Tn, n_prob)


def test_baseline_work_floats_match_library():
    from localmd_amd import baseline as BL

    lib = _lib()
    for n in (0, 1, 141, 4097):
        for cols in (0, 1, 3, 4, 255, 256, 1921):
            assert lib.pmd_sliding_extremum_work_floats(n, cols) == (n * (-(-cols // 4) * 4) if n >= 1 and cols >= 1 else 0)
            for half in (0, 1, 94):
                assert BL.quantile_work_floats(n, cols, half) == lib.pmd_sliding_quantile_work_floats(n, cols, half)
    # filter_plan: every column range's workspace, as the library sizes it, is within the plan's figure and within WORK_BYTES;
    # the largest range attains the figure
    for n_bins, N in ((1, 1), (1, 5), (141, 1921), (977, 262144), (70000, 262144), (300000, 1000), (2 ** 23 - 1, 10), (2 ** 24, 7)):
        ranges, work = BL.filter_plan(n_bins, N)
        assert ranges[0][0] == 0 and ranges[-1][1] == N and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        need = [int(lib.pmd_sliding_extremum_work_floats(n_bins, c1 - c0)) for c0, c1 in ranges]
        assert max(need) == work, (n_bins, N, max(need), work)
        assert 4 * work <= BL.WORK_BYTES or work == 4 * n_bins, (n_bins, N)


# =====================================================================================================================
# 4. everything runs on the context's stream
@pytest.fixture(scope="module")
def side(gpu_ctx):
    """A non-blocking side stream, the contexts made under it (one per environment) and their null-stream twins, and the
    cycle count of a DELAY_MS delay on this device."""
    torch = _t()

    class Side:
        pass

    s = Side()
    s.stream = torch.cuda.Stream(device=gpu_ctx.device)
    s.made = {}

    def contexts(env):
        """(context on the side stream, context on the null stream), both created under env (None: the session context)."""
        key = tuple(sorted((env or {}).items()))
        if key not in s.made:
            with torch.cuda.stream(s.stream):
                on_side = context_under(env or {})
            s.made[key] = (on_side, context_under(env) if env else gpu_ctx)
        return s.made[key]

    s.contexts = contexts
    # calibrate torch.cuda._sleep (its unit is device clock ticks)
    probe = 20_000_000
    ms = []
    with torch.cuda.stream(s.stream):
        for _ in range(2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(probe)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    assert ms[1] > 0.5, ms
    s.cycles = int(probe * DELAY_MS / ms[1])
    yield s
    for on_side, on_null in s.made.values():
        on_side.close()
        if on_null is not gpu_ctx:
            on_null.close()


def run_on_side(side, ctx, case, call=None, early_write_check=False):
    """The harness of section 4 with `ctx` (bound to side.stream).  call(): what is enqueued behind the copies, by default
    the case's own call on an exactly sized guarded workspace.  Returns the bits."""
    torch = _t()
    case.load("B")
    g = Guarded(ctx, case.nbytes, 0xFF)
    torch.cuda.synchronize()
    with torch.cuda.stream(side.stream):
        t0 = time.perf_counter()
        torch.cuda._sleep(side.cycles)
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        t1 = time.perf_counter()
        case.copy_inputs("A")
        t2 = time.perf_counter()
        pending = not ev.query()
        if call is None:
            rc = case.run(ctx, g.ptr if case.nbytes else None, case.nbytes)
        else:
            rc = call()
    assert pending, "inconclusive: the delay had ended before the call was made"
    assert rc == 0, (rc, ctx.lib.pmd_last_error(ctx.handle))
    if early_write_check:
        # nothing of an asynchronous call may have written its outputs while the delay still runs: whatever went to the
        # null stream has finished after its synchronisation, and a third stream reads the outputs
        assert not ev.query(), "inconclusive: the call outlasted the delay (it synchronises, or the delay is too short)"
        torch.cuda.default_stream().synchronize()
        third = torch.cuda.Stream()
        with torch.cuda.stream(third):
            seen = [t.clone() for t in case.outs]
        third.synchronize()
        assert not ev.query(), "inconclusive: the delay ended before the outputs were read"
        assert all(bool((t.view(torch.uint8) == T.PREFILL).all()) for t in seen), "an output was written before the delay ended"
    side.stream.synchronize()
    print(f"\n  stream harness: enqueue of the delay {1e3 * (t1 - t0):.3f} ms, of the copies {1e3 * (t2 - t1):.3f} ms")
    assert g.guards_intact()
    return case.bits()


@gpu
def test_stream_harness_detects_a_consumer_on_the_wrong_stream(gpu_ctx, cases, side):
    """Self-test: the 'call' is a torch copy of the input into the output.  Issued on the side stream it sees A; issued on
    the null stream instead it runs while the input still holds B, and the harness's comparison shows it.  The delay's
    measured duration is printed."""
    torch = _t()
    case = cases("gemm-130x70x300")
    ctx, _ = side.contexts(None)
    seen = torch.empty_like(case.ins[0])

    def good():
        seen.copy_(case.ins[0], non_blocking=True)
        return 0

    def bad():
        with torch.cuda.stream(torch.cuda.default_stream()):
            seen.copy_(case.ins[0], non_blocking=True)
        return 0

    run_on_side(side, ctx, case, call=good)
    assert torch.equal(seen, case.A[0])
    run_on_side(side, ctx, case, call=bad)
    torch.cuda.synchronize()
    assert torch.equal(seen, case.B[0]) and not torch.equal(seen, case.A[0])
    with torch.cuda.stream(side.stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(side.cycles)
        e1.record()
        e1.synchronize()
    print(f"\n  delay of {side.cycles} ticks: {e0.elapsed_time(e1):.1f} ms (target {DELAY_MS})")
    assert e0.elapsed_time(e1) > 0.5 * DELAY_MS


STREAM_ROWS = [
    # the driver's own side-stream entries
    ("chol_inverse-130-abs0", None), ("chol_inverse-641-abs0", None), ("chol_inverse-641-abs1", None), ("threshold_sim", None),
    # every distinct way the library reaches the GPU
    ("gemm-130x70x300", None), ("gemm-splitk-200x333x70001", None), ("gemm-130x70x300", F16_ENV), ("syevd-72", None),
    ("syevd-301", OWN_SYEVD_ENV), ("orthogonalize-M-200x130", None), ("projected_svd-50x300x120", None), ("gram_mtgm-217x90", None),
    ("wide_eig", None), ("background_rsvd", None), ("tiles_decompose", None),
]


# (row, environment is set) -> a kernel group that must be in the profile of the call: the route the row is there for
ROUTE_GROUP = {("gemm-130x70x300", False): "rocblas_sgemm", ("gemm-splitk-200x333x70001", False): "rocblas_sgemm_splitk",
               ("gemm-130x70x300", True): "gemm_f16x2", ("syevd-301", True): "sytrd", ("chol_inverse-130-abs0", False): "cholesky_f64",
               ("chol_inverse-641-abs0", False): "cholesky", ("chol_inverse-641-abs1", False): "cholesky"}


def profiled(ctx, case):
    """(bits, kernel groups) of the call on inputs A on ctx (bound to torch's current stream)."""
    ctx.profile_enable(True)
    try:
        rc, bits, intact, _ = run_guarded(ctx, case)
        prof = ctx.profile_summary()
    finally:
        ctx.profile_enable(False)
    assert rc == 0 and intact
    return bits, set(prof)


@gpu
@pytest.mark.parametrize("row,env", STREAM_ROWS, ids=[r + ("" if e is None else "-" + "-".join(e.values())) for r, e in STREAM_ROWS])
def test_call_runs_on_the_contexts_stream(gpu_ctx, cases, side, row, env):
    case = cases(row)
    on_side, on_null = side.contexts(env)
    ref, groups = profiled(on_null, case)
    if env is None:
        assert same_bits(ref, reference(gpu_ctx, case))
    want = ROUTE_GROUP.get((row, env is not None))
    assert want is None or want in groups, (row, env, "the row no longer reaches the route it is there for", sorted(groups))
    if env is F16_ENV:
        assert gpu_ctx.lib.pmd_gemm_split_active(gpu_ctx.handle, 130, 70, 300) == 0
    bits = run_on_side(side, on_side, case, early_write_check=(row == "threshold_sim"))
    assert same_bits(bits, ref), (row, env, "part of the call did not run on the context's stream (it saw the inputs of set B)")


def run_on_null_while_side_sleeps(side, ctx, case):
    """The call on inputs A with `ctx` on the null stream while the side stream is held by the delay: whatever still goes to
    the side stream has not run when the null stream has drained, and the bits read then show it."""
    torch = _t()
    case.load("A")
    g = Guarded(ctx, case.nbytes, 0xFF)
    torch.cuda.synchronize()
    with torch.cuda.stream(side.stream):
        torch.cuda._sleep(side.cycles)
        ev = torch.cuda.Event()
        ev.record()
    rc = case.run(ctx, g.ptr if case.nbytes else None, case.nbytes)
    torch.cuda.default_stream().synchronize()
    bits = case.bits()
    torch.cuda.default_stream().synchronize()
    assert not ev.query(), "inconclusive: the delay ended before the results were read"
    side.stream.synchronize()
    assert rc == 0 and g.guards_intact()
    return bits


@gpu
def test_ctx_set_stream_moves_every_route(gpu_ctx, cases, side):
    """Contexts created on the null stream, set to the side stream (own kernels, rocBLAS and rocSOLVER through the rocBLAS
    handle, hipBLASLt per call all follow) and set back (nothing stays behind on the side stream): the rocBLAS, split-K and
    fp16-piece routes of pmd_gemm, and pmd_chol_inverse on its fp64 and its blocked route."""
    from localmd_amd._lib import Context

    torch = _t()
    plain_rows = ["gemm-130x70x300", "gemm-splitk-200x333x70001", "chol_inverse-130-abs0", "chol_inverse-641-abs0"]
    for env, rows in ((None, plain_rows), (F16_ENV, ["gemm-130x70x300"])):
        ctx = context_under(env) if env else Context(0)
        try:
            refs = {}
            for r in rows:
                refs[r], groups = profiled(ctx, cases(r))
                assert ROUTE_GROUP[(r, env is not None)] in groups, (r, env, sorted(groups))
                assert env is not None or same_bits(refs[r], reference(gpu_ctx, cases(r)))
            assert ctx.lib.pmd_ctx_set_stream(ctx.handle, side.stream.cuda_stream) == 0
            for r in rows:
                assert same_bits(run_on_side(side, ctx, cases(r)), refs[r]), (r, env, "after pmd_ctx_set_stream(side)")
            assert ctx.lib.pmd_ctx_set_stream(ctx.handle, torch.cuda.default_stream().cuda_stream) == 0
            for r in rows:
                assert same_bits(run_on_null_while_side_sleeps(side, ctx, cases(r)), refs[r]), (r, env, "after setting the stream back")
        finally:
            ctx.close()


# =====================================================================================================================
# 5. contexts are independent; scratch trimming
@gpu
def test_two_contexts_at_once(gpu_ctx, cases):
    """The driver's Cholesky step (_cholesky_attempt): the split-K product on the main context, the blocked Cholesky chain
    on ctx.side() behind an event, joined by a second event.  Both give the bits of their solo runs."""
    torch = _t()
    ctx, sc = gpu_ctx, gpu_ctx.side()
    big, chol = cases("gemm-splitk-200x333x70001"), cases("chol_inverse-641-abs0")
    ref_big, ref_chol = reference(ctx, big), reference(ctx, chol)
    big.load("A")
    chol.load("A")
    g = Guarded(ctx, chol.nbytes, 0xFF)
    main = torch.cuda.current_stream(ctx.device)
    ev_c = torch.cuda.Event()
    ev_c.record(main)
    assert big.run(ctx, None, 0) == 0
    sc.stream.wait_event(ev_c)
    with torch.cuda.stream(sc.stream):
        assert chol.run(sc, g.ptr, chol.nbytes) == 0
    ev_e = torch.cuda.Event()
    ev_e.record(sc.stream)
    main.wait_event(ev_e)
    ctx.sync()
    assert g.guards_intact()
    assert same_bits(big.bits(), ref_big), "the product next to the Cholesky chain differs from its solo run"
    assert same_bits(chol.bits(), ref_chol), "the Cholesky chain next to the product differs from its solo run"


@gpu
def test_scratch_trim(gpu_ctx, cases):
    """pmd_scratch_trim(ctx, 0): 0 on a fresh context; after a forced fp16-piece product (two pieces of both operands of the
    200 x 333 x 70001 product: 150 MB of library-owned scratch) the device's free memory rises by at least that, and the
    same product afterwards gives the same bits."""
    torch = _t()
    m, n, k = 200, 333, 70001
    case = cases("gemm-splitk-200x333x70001")
    ctx = context_under(F16_ENV)
    try:
        assert ctx.lib.pmd_scratch_trim(ctx.handle, 0) == 0
        assert ctx.lib.pmd_gemm_split_active(ctx.handle, m, n, k) == 1
        rup8 = lambda x: (x + 7) // 8 * 8
        need = (2 * 2 * m * rup8(k) + 256) + (2 * 2 * k * rup8(n) + 256)
        rc, first, _, _ = run_guarded(ctx, case)
        assert rc == 0
        ctx.profile_enable(True)
        rc, again, _, _ = run_guarded(ctx, case)
        prof = ctx.profile_summary()
        ctx.profile_enable(False)
        assert rc == 0 and same_bits(first, again)
        assert "gemm_f16x2" in prof, sorted(prof)
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info(ctx.device)[0]
        assert ctx.lib.pmd_scratch_trim(ctx.handle, 0) == 0
        after = torch.cuda.mem_get_info(ctx.device)[0]
        assert after - before >= need, (after - before, need)
        assert ctx.lib.pmd_scratch_trim(ctx.handle, 0) == 0
        rc, third, _, _ = run_guarded(ctx, case)
        assert rc == 0 and same_bits(first, third), "the product after a trim differs"
    finally:
        ctx.close()


@gpu
@pytest.mark.parametrize("row", ["orthogonalize-M-200x130", "background_rsvd", "tiles_decompose"])
def test_fresh_context_gives_the_warmed_contexts_bits(gpu_ctx, cases, row):
    """One global, one prep and one tile row on a brand-new context against the session context, which by now has grown its
    eigensolver scratch, its split scratch and its plan cache in the tests above (and in whatever ran before this module)."""
    from localmd_amd._lib import Context

    case = cases(row)
    ref = reference(gpu_ctx, case)
    ctx = Context(0)
    try:
        rc, bits, intact, _ = run_guarded(ctx, case)
        assert rc == 0 and intact and same_bits(bits, ref), row
    finally:
        ctx.close()
