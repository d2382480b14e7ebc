"""
The percentile baseline (method="percentile" of localmd_amd.baseline, pmd_sliding_quantile) beside the extremum baseline
of scripts/baseline_probe.py.

  --part filter   the filter alone on a resident (n x N) matrix of knots (a floor with slow drift and Gaussian noise), as
                  baseline._filter runs it, device events around the calls, median of --reps after a warm-up:
                    config "4k"     625 x 262 144, half 94, q 0.08 (rank 15): the knots of DESIGN 4k
                    config "trace"  10 000 x 512, half 1500, q 0.08 (rank 240): temporal_bin=1 on 512 traces
                  with the extremum filters ("maximin": two passes) on the same matrix, and the work model: element
                  visits n min(W, n) per column for the one scan per output plus 33 scans per slice, 4 bytes each from
                  L1 / L2.  --config picks one, for a profiler run of its own.
  --part calls    whole calls at the shape of baseline_probe.py (512 x 512 x T, rank --rank), wall clock after a warm-up
                  call, median of --reps: export_movie (the yardstick), rolling_baseline and dff_movie with "maximin" and
                  with "percentile".

Prints a table and one JSON line (and writes both to --out).

    python scripts/baseline_quantile_probe.py [--part filter|calls|both] [--config 4k|trace|both] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {"4k": dict(n=625, N=512 * 512, half=94, q=0.08), "trace": dict(n=10000, N=512, half=1500, q=0.08)}


def knots_like(n, N, device, seed=0):
    import torch

    g = torch.Generator(device=device)
    g.manual_seed(seed)
    t = torch.arange(n, device=device, dtype=torch.float32)[:, None]
    return 1000.0 * (0.6 + 0.4 * torch.exp(-t / (0.4 * n))) + 3.0 * torch.randn((n, N), generator=g, device=device)


def filter_ms(ctx, K, half, method, q, reps):
    import torch
    from localmd_amd import baseline as BL

    ms = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        BL._filter(ctx, K, half, method, q)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms[1:]))


def filter_part(ctx, names, reps, lines):
    from localmd_amd import baseline as BL

    rec = {}
    lines.append("%-6s %7s %8s %5s %5s %11s %11s %12s %10s %9s" % (
        "config", "n", "N", "half", "rank", "quantile ms", "maximin ms", "visits/col", "model GB", "GB/s"))
    for name in names:
        c = CONFIGS[name]
        n, N, half, q = c["n"], c["N"], c["half"], c["q"]
        K = knots_like(n, N, ctx.device)
        W, S = 2 * half + 1, BL.QUANTILE_SLICE
        visits = (n + 33 * -(-n // S)) * min(W, n)
        nbytes = 4.0 * visits * N
        tq = filter_ms(ctx, K, half, "percentile", q, reps)
        tm = filter_ms(ctx, K, half, "maximin", None, reps)
        rec[name] = {"n": n, "N": N, "half": half, "rank": BL.percentile_rank(half, q), "column_ranges": len(BL.filter_plan(n, N)[0]),
                     "quantile_ms": tq, "maximin_ms": tm, "quantile_over_maximin": tq / tm, "visits_per_column": visits,
                     "model_bytes": nbytes, "gb_s": nbytes / (tq * 1e-3) / 1e9}
        lines.append("%-6s %7d %8d %5d %5d %11.3f %11.3f %12d %10.2f %9.1f" % (
            name, n, N, half, rec[name]["rank"], tq, tm, visits, nbytes / 1e9, rec[name]["gb_s"]))
        del K
    return rec


def calls_part(ctx, args, lines):
    import torch
    import localmd_amd
    from scripts.diag_bench import synthetic_pmd, wall

    d, T = args.d, args.T
    pmd = synthetic_pmd(d, T, args.rank)
    out = torch.empty((T, d, d), dtype=torch.float32, device=ctx.device)
    rec = {"shape": [T, d, d], "rank": args.rank, "temporal_bin": args.bin, "window": args.window}
    rec["export_denoised_s"] = wall(lambda: localmd_amd.export_movie(pmd, out, ctx=ctx), args.reps)
    for method in ("maximin", "percentile"):
        kw = dict(window=args.window, temporal_bin=args.bin, method=method, ctx=ctx)
        rec["rolling_baseline_%s_s" % method] = wall(lambda: localmd_amd.rolling_baseline(pmd, **kw), args.reps)
        rec["dff_movie_%s_s" % method] = wall(lambda: localmd_amd.dff_movie(pmd, out, **kw), args.reps)
    ctx.profile_enable(True)
    localmd_amd.dff_movie(pmd, out, window=args.window, temporal_bin=args.bin, method="percentile", ctx=ctx)
    ctx.sync()
    prof = ctx.profile_summary()
    ctx.profile_enable(False)
    rec["dff_percentile_kernel_groups_ms"] = {k: v[0] for k, v in prof.items()}
    rec["dff_percentile_kernel_ms"] = sum(v[0] for v in prof.values())
    lines.append("export %.4f s" % rec["export_denoised_s"])
    for method in ("maximin", "percentile"):
        a, b = rec["rolling_baseline_%s_s" % method], rec["dff_movie_%s_s" % method]
        lines.append("%-10s rolling_baseline %.4f s (%.2f exports), dff_movie %.4f s (%.2f exports)" % (
            method, a, a / rec["export_denoised_s"], b, b / rec["export_denoised_s"]))
    lines.append("dff_movie percentile: sliding_quantile %.3f ms of %.1f ms of kernels" % (
        prof.get("sliding_quantile", (float("nan"), 0))[0], rec["dff_percentile_kernel_ms"]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("filter", "calls", "both"), default="both")
    ap.add_argument("--config", choices=("4k", "trace", "both"), default="both")
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--rank", type=int, default=10000)
    ap.add_argument("--bin", type=int, default=16)
    ap.add_argument("--window", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from localmd_amd import decomposition as Dm
    from localmd_amd._lib import Context

    Dm.QUIET = True
    ctx = Context(0)
    lines, rec = [], {"reps": args.reps}
    if args.part in ("filter", "both"):
        rec["filter"] = filter_part(ctx, list(CONFIGS) if args.config == "both" else [args.config], args.reps, lines)
    if args.part in ("calls", "both"):
        rec["calls"] = calls_part(ctx, args, lines)
    text = "\n".join(lines) + "\n" + json.dumps(rec) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
