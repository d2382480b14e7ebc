"""
Projection onto a stored basis (localmd_amd/projection.py) at the config-3 shape: a 512 x 512 FOV, 20 x 20 tiles at
stride 10 (2 601 tiles), tile ranks drawn around the 21.4 mean of the config-3 run plus 15 dense background columns
(about 55 800 columns of U), rank 10 000 R, and a device-resident movie of --T frames in uint16 and in fp32.

Reports, per dtype: the sparse stage (pmd_group_project) time, its bytes and flops against 8 TB/s / 157 TFLOP/s, the
time of pmd_standardize_transpose_typed on the same batch (the first step of an unfused route), the R^T Z time
(pmd_gemm) and the end-to-end project_frames time on the device tensor.  Prints one JSON line.

    python scripts/project_probe.py [--T 10000] [--rank 10000] [--reps 5] [--out profiles/r05_project_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS, MFMA_TFS = 8.0, 157.0


def config3_u(d=512, b=20, stride=10, K=15, seed=0):
    rng = np.random.default_rng(seed)
    ids = np.arange(d * d).reshape(d, d, order="F")
    origins = list(range(0, d - b, stride)) + [d - b]
    rows, cols, vals = [], [], []
    j = 0
    for i0 in origins:
        for j0 in origins:
            sup = ids[i0:i0 + b, j0:j0 + b].reshape(-1)
            r = int(np.clip(rng.normal(21.4, 6.0), 1, 50))
            rows.append(np.tile(sup, r))
            cols.append(np.repeat(np.arange(j, j + r), sup.size))
            vals.append(rng.standard_normal(sup.size * r) / b)
            j += r
    for _ in range(K):
        rows.append(np.arange(d * d))
        cols.append(np.full(d * d, j))
        vals.append(rng.standard_normal(d * d) / d)
        j += 1
    u = scipy.sparse.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(d * d, j))
    return u, len(origins) ** 2


def timed(fn, reps):
    import torch

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
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--rank", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from localmd_amd import decomposition as Dm
    from localmd_amd import projection as P
    from localmd_amd._lib import Context, ptr
    from localmd_amd.pmdarray import PMDArray

    Dm.QUIET = True
    d, T = 512, args.T
    D = d * d
    t0 = time.perf_counter()
    u, n_tiles = config3_u(d)
    tabs = P.group_tables(u, (d, d), "F")
    t_tables = time.perf_counter() - t0
    n_cols = u.shape[1]
    ctx = Context(0)
    dev = ctx.device
    dt = P.DeviceTables(ctx, tabs)
    g = tabs["groups"]
    r_g, p_g = g[:, 4].astype(np.float64), g[:, 1].astype(np.float64)
    flops_useful = 2.0 * float(np.sum(r_g * p_g)) * T
    flops_mfma = 2.0 * float(np.sum(np.ceil(r_g / 16) * 16 * np.ceil(p_g / 64) * 64)) * T
    gen = torch.Generator(device=dev).manual_seed(1)
    mean = torch.full((D,), 1000.0, device=dev)
    std = torch.full((D,), 10.0, device=dev)
    rank = args.rank
    R = torch.randn((n_cols, rank), device=dev, generator=gen) / np.sqrt(n_cols)
    rs = rank
    Z = torch.empty((n_cols, T), device=dev)
    ws = torch.empty(max(dt.workspace_bytes(ctx, T), 1), dtype=torch.uint8, device=dev)
    C = torch.empty((rank, T), device=dev)
    rec = {"T": T, "D": D, "tiles": n_tiles, "groups": int(len(g)), "n_cols": int(n_cols), "rank": rank,
           "wide_groups": int(np.sum(g[:, 5])), "tables_s": round(t_tables, 2), "flops_useful": flops_useful,
           "flops_mfma": flops_mfma, "a_bytes": int(tabs["a"].nbytes)}
    for name, elem, tdt in (("uint16", 1, torch.int16), ("fp32", 0, torch.float32)):
        y32 = (1000.0 + 10.0 * torch.randn((T, D), device=dev, generator=gen)).round_()
        y = y32.to(torch.int16) if tdt == torch.int16 else y32
        del y32
        esize = 2 if elem == 1 else 4
        ms_sparse = timed(lambda: dt.project(ctx, y, elem, T, mean, std, Z, T, ws), args.reps)
        bytes_min = T * D * esize + tabs["a"].nbytes + n_cols * T * 4
        ld = int(ctx.lib.pmd_time_ld(T))
        xs = torch.empty((D, ld), device=dev)
        ms_std = timed(lambda: ctx.call("pmd_standardize_transpose_typed", ptr(y), elem, D, None, T, ptr(mean), ptr(std),
                                        ptr(xs), ld), args.reps)
        del xs
        ms_gemm = timed(lambda: ctx.call("pmd_gemm", 1, 0, rank, T, n_cols, 1.0, ptr(R), rs, ptr(Z), T, 0.0, ptr(C), T),
                        args.reps)
        pmd = PMDArray(u, np.zeros((n_cols, 1), np.float32), np.ones(1, np.float32), np.zeros((1, 1), np.float32),
                       (1, d, d), "F", np.full((d, d), 1000.0, np.float32), np.full((d, d), 10.0, np.float32))
        pmd._groups = tabs
        pmd._r = R.cpu().numpy()
        yv = y.view(T, d, d)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        pmd.project_frames(yv, frame_batch_size=T, ctx=ctx)
        ms_e2e = (time.perf_counter() - t1) * 1e3
        rec[name] = {
            "sparse_ms": round(ms_sparse, 3), "standardize_transpose_ms": round(ms_std, 3), "rtz_ms": round(ms_gemm, 3),
            "end_to_end_ms": round(ms_e2e, 1),
            "sparse_min_bytes": bytes_min, "sparse_tb_s": round(bytes_min / ms_sparse / 1e9, 3),
            "sparse_hbm_fraction": round(bytes_min / ms_sparse / 1e9 / HBM_TBS, 3),
            "sparse_useful_tflops": round(flops_useful / ms_sparse / 1e9, 2),
            "sparse_mfma_fraction": round(flops_mfma / ms_sparse / 1e9 / MFMA_TFS, 3),
            "fused_faster_than_standardize": bool(ms_sparse < ms_std),
        }
        del y
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
