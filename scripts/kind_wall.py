"""
Whole-call wall time of the five per-pixel consumers of a decomposition (summary_images, quantile_images, regressor_maps,
superpixels, rolling_baseline) at the headline shape of scripts/baseline_probe.py: a 512 x 512 FOV, the config-3-shaped
spatial basis, --T frames, and a uint16 host movie where a consumer reads one.  Per consumer: one warm-up call, then the
median of three timed calls; one process gives one sample per consumer, so trees are compared by alternating processes.
Prints one JSON line (and appends it to --out).

    python scripts/kind_wall.py [--T 10000] [--rank 200] [--tag NAME] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.diag_bench import synthetic_pmd   # noqa: E402


def host_movie(T, d, seed=2):
    """(T, d, d) uint16: one seeded 1024-frame block about 1000 with std 10, repeated."""
    rng = np.random.default_rng(seed)
    block = np.rint(1000.0 + 10.0 * rng.standard_normal((1024, d, d), dtype=np.float32)).astype(np.uint16)
    return np.concatenate([block] * -(-T // 1024))[:T]


def once(fn, reps=3):
    """The median wall time of ``reps`` calls after one warm-up call."""
    import torch

    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--rank", type=int, default=200)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import localmd_amd
    from localmd_amd import decomposition as Dm
    from localmd_amd._lib import Context

    Dm.QUIET = True
    ctx = Context(0)
    d, T = args.d, args.T
    pmd = synthetic_pmd(d, T, args.rank)
    mov = host_movie(T, d)
    x = np.random.default_rng(3).standard_normal((3, T))
    both = ("denoised", "raw")
    rec = {"tag": args.tag, "shape": [T, d, d], "rank": args.rank}
    rec["summary_images_s"] = once(lambda: localmd_amd.summary_images(pmd, mov, kinds=both, ctx=ctx))
    rec["quantile_images_s"] = once(lambda: localmd_amd.quantile_images(pmd, mov, kinds=both, ctx=ctx))
    rec["regressor_maps_s"] = once(lambda: localmd_amd.regressor_maps(pmd, x, mov, kinds=both, stat="correlation",
                                                                       ctx=ctx))
    rec["superpixels_s"] = once(lambda: localmd_amd.superpixels(pmd, kind="denoised", ctx=ctx))
    rec["rolling_baseline_s"] = once(lambda: localmd_amd.rolling_baseline(pmd, mov, kind="raw", window=3000, ctx=ctx))
    ctx.close()
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
