"""
The spatial filter (localmd_amd.spatial, csrc/spatial.hip) on one 512 x 512 x 1024 block resident in HBM, next to
pmd_shift_apply with fractional shifts on the same block (the project's read-once, write-once frame kernel: the
yardstick), and the cost of ``prefilter=`` on a whole register_movie call.

  block   band-pass at radius 3 (sigma 1.5) and 14 (sigma 7), low-pass at radius 3 (no box sums), from float32 and int16
          into float32; event times here, kernel times from ``rocprofv3 --kernel-trace --stats -- python
          scripts/spatial_bench.py --block-only``.  Bytes moved per call: (esize + 4) n D.
  call    register_movie on 512 x 512 x --T int16 frames resident on the device, max_shift 15, an explicit template, float32
          output into a device tensor, without and with ``prefilter=3``: wall clock of the second of two calls.

Prints one JSON line (and writes it to --out).

    python scripts/spatial_bench.py [--T 10000] [--reps 5] [--block-only] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.diag_bench import ev_time, movie, wall   # noqa: E402


def block(ctx, d, n, reps):
    import torch
    from localmd_amd import register as RG
    from localmd_amd import spatial as S
    from localmd_amd._lib import ptr

    D = d * d
    x32 = movie(d, n, ctx.device).reshape(n, D).contiguous()
    x16 = x32.to(torch.int16)
    out = torch.empty((n, D), dtype=torch.float32, device=ctx.device)
    rec = {"block": [n, d, d]}
    filters = {"bandpass_r3": S.spatial_filter(1.5), "bandpass_r14": S.spatial_filter(7.0),
               "lowpass_r3": S.spatial_filter(1.5, "lowpass")}
    shifts = np.random.default_rng(0).uniform(-3, 3, (n, 2))
    ish, wts = RG.shift_tables(shifts)
    ishd, wtsd = torch.from_numpy(ish).to(ctx.device), torch.from_numpy(wts).to(ctx.device)
    for tag, x, elem in (("f32", x32, 0), ("i16", x16, 2)):
        nbytes = n * D * (x.element_size() + 4)
        for name, filt in filters.items():
            ms = ev_time(lambda: S.run_filter(ctx, filt, ptr(x), elem, n, d, d, ptr(out)), reps)
            rec["%s_%s_ms" % (name, tag)] = ms
            rec["%s_%s_TBs" % (name, tag)] = nbytes / ms / 1e9
        ms = ev_time(lambda: ctx.call("pmd_shift_apply", ptr(x), elem, D, d, n, d, d, ptr(ishd), ptr(wtsd), 0, 0.0, ptr(out), 0,
                                      D, d), reps)
        rec["shift_apply_%s_ms" % tag] = ms
        rec["shift_apply_%s_TBs" % tag] = nbytes / ms / 1e9
        rec["bandpass_r3_over_shift_apply_%s" % tag] = rec["bandpass_r3_%s_ms" % tag] / ms
    return rec


def calls(ctx, d, T):
    import torch
    import localmd_amd

    mov = movie(d, T, ctx.device).to(torch.int16)
    template = mov[:100].to(torch.float32).mean(dim=0).cpu().numpy()
    out = torch.empty((T, d, d), dtype=torch.float32, device=ctx.device)
    rec = {"movie": [T, d, d]}
    for name, kw in (("plain", {}), ("prefilter3", dict(prefilter=3))):
        t = wall(lambda: localmd_amd.register_movie(mov, out, max_shift=15, template=template, ctx=ctx, **kw), 1)
        rec["register_movie_%s_s" % name] = t
    rec["prefilter_over_plain"] = rec["register_movie_prefilter3_s"] / rec["register_movie_plain_s"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--block-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from localmd_amd._lib import Context

    ctx = Context(0)
    rec = block(ctx, args.d, args.n, args.reps)
    torch.cuda.empty_cache()
    if not args.block_only:
        rec.update(calls(ctx, args.d, args.T))
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
