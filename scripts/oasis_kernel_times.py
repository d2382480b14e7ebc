"""pmd_oasis_ar1 and pmd_oasis_ar2 through the C ABI at T = 10 000, 512 and 4096 problems (8 penalties per trace): per kernel
and shape one warm-up launch, two rss-only launches and two with C, S, rss and n_pools.  The script behind profiles/oasis_ar2_kernel_stats.md:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o oasis -- python3 scripts/oasis_kernel_times.py
    python3 scripts/oasis_kernel_times_parse.py DIR        # the dispatches of both kernels in launch order, in ns"""
import importlib
import os
import sys

import numpy as np
import scipy.signal
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from localmd_amd._lib import Context, ptr as P       # noqa: E402

DX = importlib.import_module("localmd_amd.deconvolve")
T, SIGMA, RATE = 10000, 0.3, 0.015
LAMS = np.linspace(0.25, 4.0, 8).astype(np.float32)


def traces(K, g1, g2, seed):
    """(T, K) float32: events at RATE per frame, amplitudes 0.5 .. 1.5, through the AR filter, unit peak, noise SIGMA."""
    rng = np.random.default_rng(seed)
    s = (rng.random((T, K)) < RATE) * rng.uniform(0.5, 1.5, (T, K))
    c = scipy.signal.lfilter([1.0], [1.0, -g1, -g2], s, axis=0)
    imp = scipy.signal.lfilter([1.0], [1.0, -g1, -g2], np.eye(1, 200)[0])
    return (c / imp.max() + SIGMA * rng.standard_normal((T, K))).astype(np.float32)


def dev(ctx, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ctx.device)


def run(ctx, order, K):
    n = 8 * K
    idx = np.repeat(np.arange(K), 8)
    lam = np.tile(LAMS, K)
    if order == 1:
        g = np.float32(0.95)
        Y = dev(ctx, traces(K, float(g), 0.0, 1), np.float32)
        par = np.stack([np.full(n, g), lam, np.zeros(n), np.zeros(n)], axis=1)
        tab, ld, row, entry = DX.power_table(g, T)[None], T + 1, np.zeros(n), "pmd_oasis_ar1"
    else:
        g = DX.ar2_from_roots(0.95, 0.5).astype(np.float32)
        Y = dev(ctx, traces(K, float(g[0]), float(g[1]), 2), np.float32)
        par = np.stack([np.full(n, g[0]), np.full(n, g[1]), lam, np.zeros(n), np.zeros(n)], axis=1)
        tab, ld, row, entry = DX.ar2_tables(g[0], g[1], T), T + 2, np.zeros(n), "pmd_oasis_ar2"
    col, pard, rowd, tabd = dev(ctx, idx, np.int32), dev(ctx, par, np.float32), dev(ctx, row, np.int32), dev(ctx, tab, np.float32)
    Cd = torch.empty((T, n), dtype=torch.float32, device=ctx.device)
    Sd = torch.empty((T, n), dtype=torch.float32, device=ctx.device)
    rd = torch.empty(n, dtype=torch.float64, device=ctx.device)
    nd = torch.empty(n, dtype=torch.int32, device=ctx.device)
    ws = torch.empty(DX.workspace_bytes(T, n, p=order), dtype=torch.uint8, device=ctx.device)
    for full in (False, False, False, True, True):         # warm-up, rss, rss, full, full
        ctx.call(entry, P(Y), K, T, n, P(col), P(pard), P(rowd), P(tabd), ld, P(Cd) if full else None, n,
                 P(Sd) if full else None, n, P(rd), P(nd) if full else None, P(ws), ws.numel())
        ctx.sync()
    print(entry, "problems", n, "rss[:3]", rd[:3].cpu().numpy(), "mean pools", float(nd.float().mean()), flush=True)


ctx = Context(0)
for K in (64, 512):
    for order in (1, 2):
        run(ctx, order, K)
ctx.close()
