"""
pmd_pixel_stats_accumulate (csrc/stats.hip) on one block of a 512 x 512 movie: n = 1024 frames in uint16 and in fp32, the
extrema (with frame numbers) and the four power sums together, and the extrema alone, next to the same reductions
written in torch on the same buffer: ``Y.float()`` followed by ``amax``, ``amin``, ``argmax`` and the four power sums of
``Y.float() - centre`` (what a user would write without the kernel; for the extrema alone the first three).

Times are HIP events around one call, warm, median of --reps.  Per case: the bytes the call has to move (the block once,
the state it forms read and written once, the centring vector) over its time against 6.3 TB/s.  Prints a table and one
JSON line.

    python scripts/stats_probe.py [--reps 20] [--bin 1] [--out profiles/stats_probe.txt]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.3


def timed(fn, reps):
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--bin", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from localmd_amd._lib import Context, ptr

    ctx = Context(0)
    dev = ctx.device
    D, n = args.d * args.d, args.n
    gen = torch.Generator(device=dev).manual_seed(1)
    y32 = (1000.0 + 10.0 * torch.randn((n, D), device=dev, generator=gen)).round_()
    centre = y32.mean(dim=0).round_()
    rows, rec = [], {"D": D, "n": n, "bin": args.bin, "reps": args.reps, "cases": []}
    rows.append("{:>7} {:>16} {:>10} {:>10} {:>8} {:>8} {:>7}".format(
        "dtype", "forms", "kernel ms", "torch ms", "speedup", "TB/s", "of HBM"))
    for name, elem in (("uint16", 1), ("fp32", 0)):
        y = y32.to(torch.int16) if elem == 1 else y32       # uint16 values in an int16 container of the same bits
        esize = y.element_size()
        for forms, moments in (("extrema+moments", True), ("extrema", False)):
            ext = torch.empty((2, D), dtype=torch.float32, device=dev)
            arg = torch.empty((2, D), dtype=torch.int32, device=dev)
            mom = torch.zeros((4, D), dtype=torch.float64, device=dev) if moments else None

            def reset():
                ext[0].fill_(float("inf"))
                ext[1].fill_(float("-inf"))
                arg.fill_(-1)

            def call():
                ctx.call("pmd_pixel_stats_accumulate", ptr(y), elem, D, n, D, 0, args.bin, ptr(centre if moments else None),
                         ptr(ext), ptr(arg), ptr(mom))

            def ref():
                f = y.float()
                out = [f.amax(dim=0), f.amin(dim=0), f.argmax(dim=0)]
                if moments:
                    z = f - centre
                    z2 = z * z
                    out += [z.sum(dim=0), z2.sum(dim=0), (z2 * z).sum(dim=0), (z2 * z2).sum(dim=0)]
                return out

            # the two agree (one call on a fresh state; the data are integers, so with bin = 1 exactly)
            reset()
            call()
            want = ref()
            agree = {"max": bool(torch.equal(ext[1], want[0])), "min": bool(torch.equal(ext[0], want[1]))}
            if args.bin == 1:
                agree["argmax"] = bool(torch.equal(arg[1].long(), want[2]))
            if moments:
                agree["sum_z2_rel"] = float(((mom[1] - want[4].double()).abs() / want[4].double()).max())
            ms, lo, hi = timed(call, args.reps)
            ms_t, lo_t, hi_t = timed(ref, args.reps)
            nbytes = n * D * esize + 2 * (8 + 8 + (32 if moments else 0)) * D + (4 * D if moments else 0)
            case = {"dtype": name, "forms": forms, "kernel_ms": round(ms, 4), "kernel_ms_min_max": [round(lo, 4), round(hi, 4)],
                    "torch_ms": round(ms_t, 4), "torch_ms_min_max": [round(lo_t, 4), round(hi_t, 4)],
                    "speedup_over_torch": round(ms_t / ms, 2), "bytes": nbytes, "tb_s": round(nbytes / ms / 1e9, 3),
                    "hbm_fraction": round(nbytes / ms / 1e9 / HBM_TBS, 3), "agrees_with_torch": agree}
            rec["cases"].append(case)
            rows.append("{:>7} {:>16} {:>10.4f} {:>10.4f} {:>8.2f} {:>8.3f} {:>7.3f}".format(
                name, forms, ms, ms_t, ms_t / ms, case["tb_s"], case["hbm_fraction"]))
            del ext, arg, mom
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
