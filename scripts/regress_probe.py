"""
pmd_regress_accumulate (csrc/regress.hip) on one block of a 512 x 512 movie: n = 1024 frames in uint16 and in fp32 against
K = 8, 32 and 128 regressors, next to the same product written in torch on the same device,
``X @ (Y.float() - mean)`` (a conversion pass that writes an fp32 copy, then rocBLAS sgemm).

Times are HIP events around one call, warm, median of --reps.  Per case: the bytes the kernel has to move (the batch
once, the fp64 accumulators and moments read and written once, X, mean) over its time against 6.3 TB/s, and its
2 K n D flop over its time against 155 TF/s (the fp32 matrix rate), and which of the two bounds the case.  Prints a
table and one JSON line.

    python scripts/regress_probe.py [--reps 20] [--out profiles/regress_probe.txt]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS, MFMA_TFS = 6.3, 155.0


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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from localmd_amd._lib import Context, ptr

    ctx = Context(0)
    dev = ctx.device
    D, n = args.d * args.d, args.n
    gen = torch.Generator(device=dev).manual_seed(1)
    y32 = (1000.0 + 10.0 * torch.randn((n, D), device=dev, generator=gen)).round_()
    mean = y32.mean(dim=0)
    rows, rec = [], {"D": D, "n": n, "reps": args.reps, "cases": []}
    head = "{:>7} {:>4} {:>10} {:>10} {:>8} {:>8} {:>7} {:>7} {:>9} {:>8}".format(
        "dtype", "K", "kernel ms", "torch ms", "speedup", "TB/s", "of HBM", "TF/s", "of fp32mm", "bound")
    rows.append(head)
    for name, elem in (("uint16", 1), ("fp32", 0)):
        y = y32.to(torch.int16) if elem == 1 else y32       # uint16 values in an int16 container of the same bits
        esize = y.element_size()
        for K in (8, 32, 128):
            x = torch.randn((K, n), device=dev, generator=gen)
            acc = torch.zeros((K, D), dtype=torch.float64, device=dev)
            mom = torch.zeros(2 * D, dtype=torch.float64, device=dev)
            call = lambda: ctx.call("pmd_regress_accumulate", ptr(y), elem, D, n, D, ptr(mean), ptr(x), n, K, ptr(acc),  # noqa: E731
                                    D, ptr(mom))
            ref = lambda: torch.matmul(x, y.float() - mean)                                                             # noqa: E731
            # the two agree (the kernel adds into acc: compare one call on zeros)
            call()
            want = ref().double()
            err = float((acc - want).abs().max() / want.abs().max())
            ms, lo, hi = timed(call, args.reps)
            ms_t, lo_t, hi_t = timed(ref, args.reps)
            nbytes = n * D * esize + 16 * (K + 2) * D + 4 * K * n + 4 * D
            flops = 2.0 * K * n * D
            t_mem, t_mm = nbytes / (HBM_TBS * 1e12), flops / (MFMA_TFS * 1e12)
            case = {"dtype": name, "K": K, "kernel_ms": round(ms, 4), "kernel_ms_min_max": [round(lo, 4), round(hi, 4)],
                    "torch_ms": round(ms_t, 4), "torch_ms_min_max": [round(lo_t, 4), round(hi_t, 4)],
                    "speedup_over_torch": round(ms_t / ms, 2), "bytes": nbytes, "tb_s": round(nbytes / ms / 1e9, 3),
                    "hbm_fraction": round(nbytes / ms / 1e9 / HBM_TBS, 3), "tflops": round(flops / ms / 1e9, 2),
                    "fp32_matrix_fraction": round(flops / ms / 1e9 / MFMA_TFS, 3),
                    "bound": "memory" if t_mem >= t_mm else "matrix", "share_of_bound": round(max(t_mem, t_mm) * 1e3 / ms, 3),
                    "max_rel_difference_to_torch": err}
            rec["cases"].append(case)
            rows.append("{:>7} {:>4} {:>10.4f} {:>10.4f} {:>8.2f} {:>8.3f} {:>7.3f} {:>7.2f} {:>9.3f} {:>8}".format(
                name, K, ms, ms_t, ms_t / ms, case["tb_s"], case["hbm_fraction"], case["tflops"],
                case["fp32_matrix_fraction"], case["bound"]))
            del acc, mom, x
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
