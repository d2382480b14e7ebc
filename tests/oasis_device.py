"""What the device tests of pmd_oasis_ar1 (tests/test_gpu_deconvolve.py) and pmd_oasis_ar2 (tests/test_gpu_deconvolve_ar2.py)
share (test infrastructure only): the launcher of either entry point with padded, prefilled outputs and a workspace
between guard bands, the bit comparisons against an emulation's results, and the deconvolve run of a file's five traces
that several of its tests compare with."""
import ctypes as C
import importlib
from typing import NamedTuple

import numpy as np

import localmd_amd
from tests.device_util import P, _t, dev

DX = importlib.import_module("localmd_amd.deconvolve")     # the module: the package exports the function under the same name

GUARD = 512                                       # bytes of guard band on either side of the workspace
FIELDS = ("calcium", "spikes", "lam", "rss", "n_pools", "evaluations")


class Layout(NamedTuple):
    """How an entry point reads its tables: ``par`` has ``width`` columns, a problem reads ``rows`` table rows from its
    tab_row on, each of at least T + ``row_extra`` entries; a pool takes ``pool_bytes`` on the stack, the first
    ``used_bytes`` of which the solver writes (the stack is one array per word, so the spare words lie at its end)."""
    p: int
    entry: str
    width: int
    rows: int
    row_extra: int
    pool_bytes: int
    used_bytes: int


AR1 = Layout(1, "pmd_oasis_ar1", 4, 1, 1, 12, 12)
AR2 = Layout(2, "pmd_oasis_ar2", 5, 3, 2, 24, 20)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def launch(lay, ctx, Y, col, par, tab_row, tab, want="CSRN", pad=(0, 0, 0), fill=0xFF):
    """The entry point of ``lay`` on the device with the outputs named in ``want`` (C, S, Rss, N_pools) and ``pad`` extra
    columns in Y, C and S; the outputs start as NaN / -1, the workspace is exactly pool_bytes T n bytes of ``fill`` between
    two guard bands of the same fill, and the padding, the guard bands and the spare words of the pools must come back
    untouched."""
    torch = _t()
    T, K = Y.shape
    n = len(col)
    ldy, ldc, lds = K + pad[0], n + pad[1], n + pad[2]
    Yd = torch.full((T, ldy), float("nan"), dtype=torch.float32, device=ctx.device)
    Yd[:, :K] = dev(ctx, Y, np.float32)
    Cd = torch.full((T, ldc), float("nan"), dtype=torch.float32, device=ctx.device) if "C" in want else None
    Sd = torch.full((T, lds), float("nan"), dtype=torch.float32, device=ctx.device) if "S" in want else None
    rd = torch.full((n,), float("nan"), dtype=torch.float64, device=ctx.device) if "R" in want else None
    nd = torch.full((n,), -1, dtype=torch.int32, device=ctx.device) if "N" in want else None
    nbytes = lay.pool_bytes * T * n
    assert nbytes == ctx.lib.pmd_oasis_ar1_workspace_bytes(T, lay.p * n) == DX.workspace_bytes(T, n, p=lay.p)
    ws = torch.full((GUARD + nbytes + GUARD,), fill, dtype=torch.uint8, device=ctx.device)
    # named, so that the tables live until the call has run (a temporary's memory goes back to the allocator at once)
    cold, pard = dev(ctx, col, np.int32), dev(ctx, par, np.float32)
    rowd, tabd = dev(ctx, tab_row, np.int32), dev(ctx, tab, np.float32)
    assert int(cold.min()) >= 0 and int(cold.max()) < K and par.shape == (n, lay.width)
    assert int(rowd.min()) >= 0 and int(rowd.max()) + lay.rows <= tab.shape[0] and tab.shape[1] >= T + lay.row_extra
    ctx.call(lay.entry, P(Yd), ldy, T, n, P(cold), P(pard), P(rowd), P(tabd), tab.shape[1], P(Cd), ldc, P(Sd), lds,
             P(rd), P(nd), C.c_void_p(ws.data_ptr() + GUARD), nbytes)
    ctx.sync()
    assert bool((ws[:GUARD] == fill).all().item()) and bool((ws[GUARD + nbytes:] == fill).all().item()), "guard band written"
    spare = ws[GUARD + lay.used_bytes * T * n:GUARD + nbytes]
    assert bool((spare == fill).all().item()), "the spare word of the pools was written"
    out = {}
    for name, t in (("C", Cd), ("S", Sd)):
        if t is not None:
            assert bool(torch.isnan(t[:, n:]).all().item()), name + ": columns beyond n_prob were written"
            out[name] = t[:, :n].cpu().numpy()
    if rd is not None:
        out["R"] = rd.cpu().numpy()
    if nd is not None:
        out["N"] = nd.cpu().numpy()
    return out


def assert_same(got, ref, names="CSRN"):
    Ce, Se, rss, npl = ref
    if "N" in names:
        assert np.array_equal(got["N"], npl), np.nonzero(got["N"] != npl)[0][:5]
    if "C" in names:
        assert np.array_equal(bits(got["C"]), bits(Ce)), "calcium: {} values differ".format(np.sum(bits(got["C"]) != bits(Ce)))
    if "S" in names:
        assert np.array_equal(bits(got["S"]), bits(Se)), "spikes: {} values differ".format(np.sum(bits(got["S"]) != bits(Se)))
    if "R" in names:
        assert np.array_equal(got["R"].view(np.int64), rss.view(np.int64)), (got["R"] - rss)


_FIVE = {}


def five_run(ctx, y, p):
    """deconvolve(p=p) of a file's five traces ``y`` with 3 rounds of 4 and the default cap, computed once per order."""
    if p not in _FIVE:
        _FIVE[p] = localmd_amd.deconvolve(y, search_rounds=3, search_points=4, ctx=ctx, p=p)
    return _FIVE[p]


def assert_result(dc, ref):
    assert np.array_equal(bits(dc.calcium), bits(ref["calcium"]))
    assert np.array_equal(bits(dc.spikes), bits(ref["spikes"]))
    assert np.array_equal(bits(dc.lam), bits(ref["lam"]))
    assert np.array_equal(dc.rss, ref["rss"])
    assert np.array_equal(dc.n_pools, ref["n_pools"])
    assert np.array_equal(dc.evaluations, ref["evaluations"])
