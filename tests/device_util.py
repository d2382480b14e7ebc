"""Small helpers the device tests of the launch cuts and of the large offsets share (test infrastructure only)."""
import numpy as np

ELEM = {"float32": 0, "uint16": 1, "int16": 2}      # PMD_ELEM_* of a container
PRE32 = 0x7FC12345                                  # the sentinel of float32 outputs: a NaN with a payload no arithmetic produces
PRE64 = 0x7FF8000012345678                          # the same for float64 outputs


def _t():
    import torch

    return torch


def P(t):
    from localmd_amd._lib import ptr

    return ptr(t)


def dev(ctx, a, dtype=None):
    return _t().from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ctx.device)


def prefilled(ctx, shape, double=False):
    torch = _t()
    if double:
        return torch.full(shape, PRE64, dtype=torch.int64, device=ctx.device).view(torch.float64)
    return torch.full(shape, PRE32, dtype=torch.int32, device=ctx.device).view(torch.float32)


def kept(t):
    """the sentinel is still there, to the bit, in all of t"""
    torch = _t()
    if t.dtype == torch.float64:
        return bool((t.view(torch.int64) == PRE64).all().item())
    return bool((t.view(torch.int32) == PRE32).all().item())
