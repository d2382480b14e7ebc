"""
ROI traces (localmd_amd.extract_traces) at the headline shape: a 512 x 512 x 10 000 integer-valued movie resident on the
device as float32 and as uint16, its decomposition (20 x 20 blocks, reference-default arguments, factors kept on the
device with to_device()), 1 000 disc masks of about 150 pixels at seeded positions plus one whole-field mask.

Times, each with a device synchronise inside the clock, median and range of --reps repeats after a warm-up call:
  - extract_traces with all three kinds (uint16 and float32 movie) and with "denoised" only;
  - in the same run, the route without extract_traces: export_movie of the "denoised" (and "raw") panel into a
    T x d x d device tensor followed by torch.sparse.mm with the same W, and torch.sparse.mm on the resident float32
    movie itself;
and the largest difference between the two routes' traces.  Prints one JSON line (and writes it to --out).
``--gather-only`` runs just the raw traces a few times: the target of the separate
``rocprofv3 --kernel-trace --stats`` run, whose roi_gather_kernel time gives the achieved algorithmic bytes/s
nnz(W) T esize / time (printed here as "gather_algorithmic_bytes").

    python scripts/traces_bench.py [--d 512] [--T 10000] [--masks 1000] [--reps 5] [--out FILE] [--gather-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ACHIEVABLE_TBS = 6.3


def disc_masks(d, n_masks, radius, seed):
    """(n_masks + 1) x d^2 boolean CSR in C pixel order: discs at seeded centres, then the whole field."""
    rng = np.random.default_rng(seed)
    r = int(np.ceil(radius))
    di, dj = np.mgrid[-r:r + 1, -r:r + 1]
    keep = di * di + dj * dj <= radius * radius
    di, dj = di[keep], dj[keep]
    ci = rng.integers(r, d - r, n_masks)
    cj = rng.integers(r, d - r, n_masks)
    rows = np.repeat(np.arange(n_masks), di.size)
    cols = ((ci[:, None] + di[None, :]) * d + (cj[:, None] + dj[None, :])).reshape(-1)
    rows = np.concatenate([rows, np.full(d * d, n_masks)])
    cols = np.concatenate([cols, np.arange(d * d)])
    return scipy.sparse.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(n_masks + 1, d * d))


def timed(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--masks", type=int, default=1000)
    ap.add_argument("--radius", type=float, default=6.9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gather-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import localmd_amd
    from localmd_amd import decomposition as Dm
    from localmd_amd._lib import Context
    from localmd_amd.synthetic import make_movie_torch

    Dm.QUIET = True
    ctx = Context(0)
    dev = ctx.device
    d, T = args.d, args.T
    D = d * d
    mov32 = torch.round(make_movie_torch(T, d, d, dev, seed=0) * 10.0 + 500.0).clamp_(0, 32767)
    mov16 = mov32.to(torch.int16).view(torch.uint16)             # the same values in a uint16 container
    Wc = disc_masks(d, args.masks, args.radius, seed=1)
    Wc = scipy.sparse.csr_matrix(Wc.multiply(1.0 / Wc.sum(axis=1)))          # reduce="mean", C pixel order
    nnz = int(Wc.nnz)
    rec = {"shape": [T, d, d], "masks": Wc.shape[0], "nnz_w": nnz, "pixels_per_disc": int(Wc[0].nnz)}
    rec["gather_algorithmic_bytes"] = {"uint16": nnz * T * 2, "float32": nnz * T * 4}
    rec["gather_floor_ms_at_6.3TBs"] = {k: v / (HBM_ACHIEVABLE_TBS * 1e12) * 1e3
                                        for k, v in rec["gather_algorithmic_bytes"].items()}

    if args.gather_only:
        # no decomposition needed for the raw traces: an empty one of the movie's shape carries the geometry
        from localmd_amd.pmdarray import PMDArray

        pmd = PMDArray(scipy.sparse.csr_matrix((D, 0)), np.zeros((0, 0), np.float32), np.zeros(0, np.float32),
                       np.zeros((0, T), np.float32), (T, d, d), "C", np.zeros((d, d), np.float32), np.ones((d, d), np.float32))
        for mov in (mov16, mov32, mov16, mov32):
            localmd_amd.extract_traces(pmd, Wc, mov, kinds="raw", reduce="sum", ctx=ctx)
        print(json.dumps(rec))
        ctx.close()
        return

    np.random.seed(0)
    pmd = localmd_amd.localmd_decomposition(mov32, (20, 20), T, max_components=50, seed=2024, ctx=ctx)
    rec["n_cols"], rec["rank"] = int(pmd.u.shape[1]), int(pmd.r.shape[1])
    # the masks with columns in the decomposition's pixel order (the sparse form of extract_traces)
    u_of_c = np.asarray(pmd.row_indices).reshape(-1)
    coo = Wc.tocoo()
    rois = scipy.sparse.csr_matrix((coo.data, (coo.row, u_of_c[coo.col])), shape=Wc.shape)
    pmd.to_device(ctx=ctx)

    out = {}

    def new(kinds, mov):
        out["new"] = localmd_amd.extract_traces(pmd, rois, mov, kinds=kinds, reduce="sum", ctx=ctx)

    rec["traces_all_uint16"] = timed(lambda: new(("denoised", "raw", "residual"), mov16), args.reps)
    rec["traces_all_float32"] = timed(lambda: new(("denoised", "raw", "residual"), mov32), args.reps)
    tr_all = out["new"]
    rec["traces_raw_uint16"] = timed(lambda: new(("raw",), mov16), args.reps)
    rec["traces_denoised"] = timed(lambda: new(("denoised",), None), args.reps)

    # the route without extract_traces, same commit, same run
    ci = torch.from_numpy(np.stack([coo.row, coo.col]).astype(np.int64)).to(dev)
    Wt = torch.sparse_coo_tensor(ci, torch.from_numpy(coo.data.astype(np.float32)).to(dev), Wc.shape).coalesce()
    buf = torch.empty((T, d, d), dtype=torch.float32, device=dev)

    def old(panel, mov):
        localmd_amd.export_movie(pmd, buf, mov, panels=panel, ctx=ctx)
        out["old"] = torch.sparse.mm(Wt, buf.reshape(T, D).t()).cpu().numpy()

    def old_direct():
        out["old"] = torch.sparse.mm(Wt, mov32.reshape(T, D).t()).cpu().numpy()

    for name, fn, ref in (("export_denoised_then_spmm", lambda: old("denoised", None), tr_all.denoised),
                          ("export_raw_then_spmm", lambda: old("raw", mov16), tr_all.raw),
                          ("spmm_on_resident_float32_movie", old_direct, tr_all.raw)):
        try:
            rec[name] = timed(fn, args.reps)
            rec[name]["max_abs_diff_to_extract_traces"] = float(np.abs(out["old"] - ref).max())
            rec[name]["max_abs_value"] = float(np.abs(ref).max())
        except Exception as e:      # noqa: BLE001 - a route torch cannot run is part of the record
            rec[name] = {"error": "{}: {}".format(type(e).__name__, e)}
    for a, b in (("traces_denoised", "export_denoised_then_spmm"), ("traces_raw_uint16", "export_raw_then_spmm"),
                 ("traces_raw_uint16", "spmm_on_resident_float32_movie")):
        if "median_s" in rec.get(b, {}):
            rec["speedup_%s_over_%s" % (a, b)] = rec[b]["median_s"] / rec[a]["median_s"]
    pmd.to_host()
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
