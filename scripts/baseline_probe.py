"""
Rolling-baseline dF/F (localmd_amd.baseline) at the headline shape of scripts/export_bench.py: a 512 x 512 FOV, the
config-3-shaped spatial basis, R with --rank columns, Vt (--rank x --T).

Reports
  - whole calls, wall clock after one warm-up call: dff_movie(kind="denoised") into a device tensor, rolling_baseline,
    and export_movie(panels="denoised") into a device tensor (existing code, the yardstick: dff_movie is two expansion
    passes plus streams over 1 / temporal_bin of the data);
  - the three kernels of csrc/baseline.hip inside one dff_movie call (HIP events around every launch, pmd_profile_*),
    with the bytes of the traffic model of DESIGN and the rate they come to:
      bin_means         reads the block once and writes 1 / temporal_bin of it
      sliding_extremum  per filter pass: two reads of the knots, one write and one read of the workspace, one write
      baseline_apply    reads the block and (from cache, not counted) the knots, writes the block
Prints a table and one JSON line (and writes both to --out).

    python scripts/baseline_probe.py [--T 10000] [--rank 10000] [--bin 16] [--window 3000] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.diag_bench import HBM_TBS, synthetic_pmd, wall   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--rank", type=int, default=10000)
    ap.add_argument("--bin", type=int, default=16)
    ap.add_argument("--window", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import localmd_amd
    from localmd_amd import baseline as BL
    from localmd_amd import decomposition as Dm
    from localmd_amd._lib import Context

    Dm.QUIET = True
    ctx = Context(0)
    d, T, b = args.d, args.T, args.bin
    D = d * d
    pmd = synthetic_pmd(d, T, args.rank)
    out = torch.empty((T, d, d), dtype=torch.float32, device=ctx.device)
    kw = dict(window=args.window, temporal_bin=b, ctx=ctx)
    rec = {"shape": [T, d, d], "rank": args.rank, "temporal_bin": b, "window": args.window,
           "half": BL.half_window(args.window, b), "reps": args.reps}
    rec["export_denoised_s"] = wall(lambda: localmd_amd.export_movie(pmd, out, ctx=ctx), args.reps)
    rec["rolling_baseline_s"] = wall(lambda: localmd_amd.rolling_baseline(pmd, **kw), args.reps)
    rec["dff_movie_s"] = wall(lambda: localmd_amd.dff_movie(pmd, out, **kw), args.reps)
    rec["dff_over_export"] = rec["dff_movie_s"] / rec["export_denoised_s"]

    ctx.profile_enable(True)
    localmd_amd.dff_movie(pmd, out, **kw)
    ctx.sync()
    prof = ctx.profile_summary()
    ctx.profile_enable(False)
    n_bins = -(-T // b)
    model = {"bin_means": 4.0 * T * D * (1 + 1.0 / b), "sliding_extremum": 2 * 5 * 4.0 * n_bins * D,
             "baseline_apply": 2 * 4.0 * T * D}
    lines = ["%-18s %8s %10s %10s %8s %8s" % ("kernel", "launches", "ms", "model GB", "GB/s", "of HBM")]
    rec["kernels"] = {}
    for name, nbytes in model.items():
        ms, cnt = prof.get(name, (float("nan"), 0))
        rate = nbytes / (ms * 1e-3) / 1e9
        rec["kernels"][name] = {"launches": cnt, "ms": ms, "model_bytes": nbytes, "gb_s": rate,
                                "hbm_fraction": rate / (HBM_TBS * 1e3)}
        lines.append("%-18s %8d %10.3f %10.3f %8.1f %8.3f" % (name, cnt, ms, nbytes / 1e9, rate, rate / (HBM_TBS * 1e3)))
    rec["other_kernel_groups_ms"] = {k: v[0] for k, v in prof.items() if k not in model}
    lines.append("export %.4f s, rolling_baseline %.4f s, dff_movie %.4f s (%.2f exports)" % (
        rec["export_denoised_s"], rec["rolling_baseline_s"], rec["dff_movie_s"], rec["dff_over_export"]))
    text = "\n".join(lines) + "\n" + json.dumps(rec) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
