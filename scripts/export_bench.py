"""
Streamed export (localmd_amd.export_movie) at the config-3 shape of scripts/diag_bench.py: a 512 x 512 FOV, the
config-3-shaped spatial basis of scripts/project_probe.py (54 604 columns), R with --rank columns, Vt (--rank x --T),
and the synthetic movie of diag_bench.

Reports
  - one 1024-frame block: pmd_gemm, pmd_group_expand (fp32 triptych, uint16 denoised only) and the existing
    pmd_csr_rows_spmm + pmd_transpose_affine pair on the same block, and the fused kernel against its floor (output and
    raw bytes at 8 TB/s, or the block's MACs at the fp32 MFMA peak, whichever is larger);
  - whole calls: denoised fp32 into a device tensor (frames/s); into a host NumPy array against the pinned
    device-to-host rate measured here; into a TIFF on local disk against a plain sequential write of the same bytes.
Prints one JSON line (and writes it to --out).  Kernel times for the record come from a separate
``rocprofv3 --kernel-trace --stats`` run of ``--phases-only``.

    python scripts/export_bench.py [--T 10000] [--rank 10000] [--host-T 4000] [--tiff-T 2000] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.diag_bench import HBM_TBS, ev_time, movie, synthetic_pmd, wall   # noqa: E402

MFMA_F32_TFLOPS = 157.3      # MI355X dense fp32 matrix-core peak


def phases(ctx, pmd, mov_dev, reps):
    """Times (ms) of one 1024-frame block: the product, the fused kernel, the pair it replaces."""
    import ctypes as C

    import torch
    from localmd_amd import export as E
    from localmd_amd._lib import ptr

    T, d1, d2 = pmd.shape
    D = d1 * d2
    n = min(E.EXPORT_BLOCK, T)
    tabs, xt = E.expand_tables_for(pmd)
    pmd.to_device(ctx=ctx)
    dv = pmd._dev
    dev = ctx.device
    n_cols, rank = dv["rs"].shape
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
    mean, std = f32(pmd.mean_img.reshape(-1)), f32(pmd.var_img.reshape(-1))
    sel = torch.from_numpy(np.ascontiguousarray(pmd.row_indices.reshape(-1), dtype=np.int32)).to(dev)
    pp = torch.from_numpy(xt["patch_ptr"]).to(dev)
    ent = torch.from_numpy(xt["entries"].reshape(-1)).to(dev)
    qm = torch.from_numpy(xt["qmap"]).to(dev)
    A = f32(tabs["a"])
    n_ent = len(xt["entries"])
    ct = torch.zeros((n_cols, n), dtype=torch.float32, device=dev)
    acc = torch.empty((D, n), dtype=torch.float32, device=dev)
    W = torch.empty((n, D), dtype=torch.float32, device=dev)
    y = mov_dev[:n].reshape(n, D).contiguous()
    out3 = torch.empty(n * D * 3, dtype=torch.float32, device=dev)
    out16 = torch.empty(n * D, dtype=torch.int16, device=dev)
    rec = {"block_frames": n, "entries": n_ent, "patches": int(xt["n_patches"])}
    rec["gemm_ms"] = ev_time(lambda: ctx.call("pmd_gemm", 0, 0, n_cols, n, rank, 1.0, ptr(dv["rs"]), rank, ptr(dv["v"]), T,
                                              0.0, ptr(ct), n), reps)

    def pair():
        ctx.call("pmd_csr_rows_spmm", ptr(dv["indptr"]), ptr(dv["indices"]), ptr(dv["data"]), ptr(sel), D, ptr(ct), n, n,
                 ptr(acc), n)
        ctx.call("pmd_transpose_affine", ptr(acc), n, D, n, ptr(std), ptr(mean), ptr(W), D)
    rec["pair_ms"] = ev_time(pair, reps)

    def fused(out, panels, code, out_elem, yp):
        ctx.call("pmd_group_expand", ptr(ct), n, n, d1, d2, ptr(mean), ptr(std), int(xt["n_patches"]), ptr(pp), n_ent,
                 ptr(ent), ptr(qm), ptr(A), yp, 0, D, panels, code, ptr(out), out_elem)
    rec["fused_triptych_f32_ms"] = ev_time(lambda: fused(out3, 3, 0 | (1 << 2) | (2 << 4), 0, C.c_void_p(y.data_ptr())),
                                           reps)
    rec["fused_denoised_u16_ms"] = ev_time(lambda: fused(out16, 1, 1, 1, None), reps)
    # MACs: every entry contracts its rows (rounded to 4) for 64 pixels and every frame
    r4 = (xt["entries"][:, 2] + 3) // 4 * 4
    macs_issued = float(r4.sum()) * 64 * n
    macs_useful = float(pmd.u.nnz) * n
    for name, nbytes in (("triptych_f32", n * D * (3 * 4 + 4)), ("denoised_u16", n * D * 2)):
        ms = rec["fused_%s_ms" % name]
        t_bytes = nbytes / (HBM_TBS * 1e12) * 1e3
        t_flop = 2 * macs_issued / (MFMA_F32_TFLOPS * 1e12) * 1e3
        rec["fused_%s_floor_ms" % name] = max(t_bytes, t_flop)
        rec["fused_%s_floor_bound" % name] = "bytes" if t_bytes >= t_flop else "mfma"
        rec["fused_%s_of_floor" % name] = max(t_bytes, t_flop) / ms
    rec["gflop_issued"] = 2 * macs_issued / 1e9
    rec["gflop_useful"] = 2 * macs_useful / 1e9
    rec["fused_over_pair"] = rec["fused_triptych_f32_ms"] / rec["pair_ms"]
    pmd.to_host()
    return rec


def d2h_rate(dev, nbytes=1 << 30):
    import torch

    h = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    g = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return nbytes / wall(lambda: h.copy_(g, non_blocking=True), 3) / 1e9


def disk_rate(path, nbytes, chunk=64 << 20):
    buf = np.random.default_rng(0).integers(0, 255, chunk, dtype=np.uint8)
    t0 = time.perf_counter()
    with open(path, "wb") as f:
        left = nbytes
        while left > 0:
            k = min(chunk, left)
            f.write(memoryview(buf)[:k])
            left -= k
        f.flush()
        os.fsync(f.fileno())
    t = time.perf_counter() - t0
    os.remove(path)
    return nbytes / t / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--rank", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-T", type=int, default=4000)
    ap.add_argument("--tiff-T", type=int, default=2000)
    ap.add_argument("--phases-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import localmd_amd
    from localmd_amd._lib import Context
    from localmd_amd import decomposition as Dm

    Dm.QUIET = True
    ctx = Context(0)
    dev = ctx.device
    rec = {"shape": [args.T, args.d, args.d], "rank": args.rank}
    pmd = synthetic_pmd(args.d, args.T, args.rank)
    rec["n_cols"] = int(pmd.u.shape[1])
    mov_dev = movie(args.d, min(args.T, 1024), dev)
    rec.update(phases(ctx, pmd, mov_dev, args.reps))
    del mov_dev
    torch.cuda.empty_cache()
    if not args.phases_only:
        d = args.d
        out = torch.empty((args.T, d, d), dtype=torch.float32, device=dev)
        t = wall(lambda: localmd_amd.export_movie(pmd, out, ctx=ctx), 1)
        rec["device_dest_s"] = t
        rec["device_dest_frames_per_s"] = args.T / t
        del out
        torch.cuda.empty_cache()
        rec["pinned_d2h_GBs"] = d2h_rate(dev)
        hp = synthetic_pmd(d, args.host_T, args.rank)
        host = np.empty((args.host_T, d, d), np.float32)
        host.fill(0)                        # touch the pages first: the rate is the copy's, not the page faults'
        t = wall(lambda: localmd_amd.export_movie(hp, host, ctx=ctx), 1)
        rec["host_dest_T"] = args.host_T
        rec["host_dest_s"] = t
        rec["host_dest_GBs"] = host.nbytes / t / 1e9
        rec["host_dest_fraction_of_pinned"] = rec["host_dest_GBs"] / rec["pinned_d2h_GBs"]
        del host
        tp = synthetic_pmd(d, args.tiff_T, args.rank)
        tmp = tempfile.mkdtemp()
        path = os.path.join(tmp, "export.tif")
        nbytes = args.tiff_T * d * d * 4
        rec["disk_write_GBs"] = disk_rate(os.path.join(tmp, "plain.bin"), nbytes)

        def tiff():
            localmd_amd.export_movie(tp, path, ctx=ctx)
            with open(path, "rb+") as f:
                os.fsync(f.fileno())
        t = wall(tiff, 1)
        os.remove(path)
        os.rmdir(tmp)
        rec["tiff_T"] = args.tiff_T
        rec["tiff_s"] = t
        rec["tiff_GBs"] = nbytes / t / 1e9
        rec["tiff_fraction_of_disk"] = rec["tiff_GBs"] / rec["disk_write_GBs"]
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
