"""
pmd_pixel_hist_accumulate / pmd_pixel_hist_select (csrc/quantile.hip) on one block of a 512 x 512 movie: n = 1024 and
n = 10000 frames in uint16 and in fp32.  Timed: the first pass (every element counted), a later pass (pass 1 with the
prefix the median's first select leaves), and the select kernel on the first pass's counts; next to them, in the same
process, pmd_pixel_stats_accumulate (extrema and the four power sums, 1024 frames per call) over the same block: the
memory-bound yardstick.

Times are HIP events around the calls, warm, median of --reps.  Per case: the bytes of the block over the time (the
histogram traffic of the flush is not counted), against 6.3 TB/s, and the ratio to the yardstick.  Prints a table and one
JSON line.

    python scripts/quantile_probe.py [--reps 10] [--out profiles/quantile_probe.txt]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.3


def timed(fn, reps, prep=None):
    import torch

    for _ in range(2):
        if prep:
            prep()
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        if prep:
            prep()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--n", type=int, nargs="+", default=[1024, 10000])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from localmd_amd._lib import Context, ptr

    ctx = Context(0)
    dev = ctx.device
    D = args.d * args.d
    G = -(-D // 64)
    rows, rec = [], {"D": D, "reps": args.reps, "cases": []}
    rows.append("{:>7} {:>6} {:>12} {:>10} {:>8} {:>7} {:>10}".format(
        "dtype", "n", "what", "ms", "GB/s", "of HBM", "/yardstick"))
    for n in args.n:
        gen = torch.Generator(device=dev).manual_seed(1)
        y32 = torch.empty((n, D), dtype=torch.float32, device=dev)
        for a in range(0, n, 1024):                        # in pieces: no second copy of a 10 GB block
            y32[a:a + 1024].normal_(1000.0, 10.0, generator=gen).round_()
        for name, elem in (("uint16", 1), ("fp32", 0)):
            y = y32.to(torch.int16) if elem == 1 else y32       # uint16 values in an int16 container of the same bits
            esize = y.element_size()
            hist = torch.zeros(G * 256 * 64, dtype=torch.int32, device=dev)
            saved = torch.empty_like(hist)
            rank = torch.empty(D, dtype=torch.int32, device=dev)
            prefix = torch.zeros(D, dtype=torch.int32, device=dev)
            prefix1 = torch.empty_like(prefix)
            centre = y32[:1024].mean(dim=0).round_()
            ext = torch.empty((2, D), dtype=torch.float32, device=dev)
            arg = torch.empty((2, D), dtype=torch.int32, device=dev)
            mom = torch.zeros((4, D), dtype=torch.float64, device=dev)
            ext[0].fill_(float("inf"))
            ext[1].fill_(float("-inf"))

            def accumulate(p, pre):
                ctx.call("pmd_pixel_hist_accumulate", ptr(y), elem, D, n, D, None, p, ptr(pre), ptr(hist))

            def select():
                ctx.call("pmd_pixel_hist_select", D, ptr(hist), ptr(rank), ptr(prefix))

            def yardstick():
                for a in range(0, n, 1024):
                    m = min(1024, n - a)
                    ctx.call("pmd_pixel_stats_accumulate", C.c_void_p(y.data_ptr() + a * D * esize), elem, D, m, D, a, 1,
                             ptr(centre), ptr(ext), ptr(arg), ptr(mom))

            def fresh_select():
                hist.copy_(saved)
                rank.fill_(n // 2)
                prefix.zero_()

            # the counts of the first pass, kept for the select runs; the prefix of the median after it; and one full
            # selection checked against torch
            hist.zero_()
            accumulate(0, None)
            saved.copy_(hist)
            assert int(saved.sum(dtype=torch.int64)) == n * D
            fresh_select()
            select()
            prefix1.copy_(prefix)
            for p in (1, 2, 3):
                accumulate(p, prefix)
                select()
            ctx.sync()
            bits = prefix.cpu().numpy().view(np.uint32)
            got = np.where(bits & 0x80000000, bits ^ np.uint32(0x80000000), ~bits).astype(np.uint32).view(np.float32)
            want = y32[:, :4096].sort(dim=0).values[n // 2].cpu().numpy()
            agree = bool(np.array_equal(got[:4096], want))

            hist.zero_()
            t_y = timed(yardstick, args.reps)
            cases = [("yardstick", t_y),
                     ("pass 0", timed(lambda: accumulate(0, None), args.reps, hist.zero_)),
                     ("later pass", timed(lambda: accumulate(1, prefix1), args.reps, hist.zero_)),
                     ("select", timed(select, args.reps, fresh_select))]
            nbytes = n * D * esize
            for what, (ms, lo, hi) in cases:
                moved = 2 * 4 * G * 256 * 64 if what == "select" else nbytes
                case = {"dtype": name, "n": n, "what": what, "ms": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)],
                        "bytes": moved, "gb_s": round(moved / ms / 1e6, 1), "hbm_fraction": round(moved / ms / 1e9 / HBM_TBS, 3),
                        "ratio_to_yardstick": round(ms / t_y[0], 2), "median_agrees_with_torch_sort": agree}
                rec["cases"].append(case)
                rows.append("{:>7} {:>6} {:>12} {:>10.4f} {:>8.1f} {:>7.3f} {:>10.2f}".format(
                    name, n, what, ms, case["gb_s"], case["hbm_fraction"], case["ratio_to_yardstick"]))
            del y, hist, saved, ext, arg, mom
        del y32
        torch.cuda.empty_cache()
    table = "\n".join(rows)
    print(table)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n" + line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
