"""
One-pass fit diagnostics (localmd_amd.make_pmd_diagnostic_images) at the config-3 shape: a 512 x 512 FOV, the
config-3-shaped spatial basis of scripts/project_probe.py (2 601 tiles of 20 x 20 at stride 10 with ranks around 21.4,
plus 15 dense background columns, F order), R with --rank columns, Vt (--rank x --T) and a movie of --T frames from the
synthetic model (make_movie_torch).

Reports
  - the phases of one reconstruction block on the device tensor (pmd_gemm, pmd_csr_rows_spmm + pmd_transpose_affine,
    pmd_diag_fused_accumulate) and the fused kernel's bytes against 8 TB/s;
  - whole calls on a device tensor, a host NumPy fp32 array and a host NumPy uint16 array, the host ones against the
    pinned host-to-device rate measured here;
  - at --small-d x --small-d x --small-T, the whole call against the four existing routines on a to_device() PMDArray.
Prints one JSON line (and writes it to --out).

    python scripts/diag_bench.py [--T 10000] [--rank 10000] [--reps 3] [--out profiles/r06_diag_bench_512x512x10000.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 8.0


def synthetic_pmd(d, T, rank, seed=0):
    from localmd_amd.pmdarray import PMDArray
    from scripts.project_probe import config3_u

    rng = np.random.default_rng(seed)
    u, _ = config3_u(d=d) if d == 512 else _small_u(d)
    n_cols = u.shape[1]
    r = (rng.standard_normal((n_cols, rank)) / np.sqrt(n_cols)).astype(np.float32)
    s = np.sort(rng.uniform(1.0, 50.0, rank))[::-1].astype(np.float32)
    v = (rng.standard_normal((rank, T)) / np.sqrt(T)).astype(np.float32)
    mean = (1000.0 + rng.uniform(-20, 20, (d, d))).astype(np.float32)
    std = rng.uniform(5.0, 15.0, (d, d)).astype(np.float32)
    return PMDArray(u.tocoo(), r, s, v, (T, d, d), "F", mean, std)


def _small_u(d):
    from scripts.project_probe import config3_u

    u, n = config3_u(d=d, K=3)
    return u, n


def movie(d, T, dev):
    import torch
    from localmd_amd.synthetic import make_movie_torch

    m = make_movie_torch(T, d, d, dev, seed=1)
    return torch.round(m * 10.0 + 500.0).clamp_(0, 65535)


def ev_time(fn, reps):
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


def wall(fn, reps):
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


def phases(ctx, pmd, mov_dev, reps):
    """Times (ms) of the three steps of one DIAG_RECON_FRAMES block, as make_pmd_diagnostic_images runs them."""
    import torch
    from localmd_amd._lib import ptr
    from localmd_amd import diagnostic_images as DI

    T, d1, d2 = pmd.shape
    D = d1 * d2
    n = min(DI.DIAG_RECON_FRAMES, T)
    ldc = (n + 3) // 4 * 4
    pmd.to_device(ctx=ctx)
    dv = pmd._dev
    n_cols, rank = dv["rs"].shape
    sel = torch.from_numpy(np.ascontiguousarray(pmd.row_indices.reshape(-1), dtype=np.int32)).to(ctx.device)
    std = torch.from_numpy(np.ascontiguousarray(pmd.var_img, dtype=np.float32).reshape(-1)).to(ctx.device)
    mean = torch.from_numpy(np.ascontiguousarray(pmd.mean_img, dtype=np.float32).reshape(-1)).to(ctx.device)
    ct = torch.zeros((n_cols, ldc), dtype=torch.float32, device=ctx.device)
    acc = torch.empty((D, ldc), dtype=torch.float32, device=ctx.device)
    W = torch.empty((n, D), dtype=torch.float32, device=ctx.device)
    ws = torch.empty(int(ctx.lib.pmd_diag_fused_workspace_bytes(n, D)), dtype=torch.uint8, device=ctx.device)
    mom = torch.zeros((35, D), dtype=torch.float64, device=ctx.device)
    ref = torch.empty((3, D), dtype=torch.float32, device=ctx.device)
    fss = torch.empty(T, dtype=torch.float64, device=ctx.device)
    out = {}
    out["gemm_ms"] = ev_time(lambda: ctx.call("pmd_gemm", 0, 0, n_cols, n, rank, 1.0, ptr(dv["rs"]), rank, ptr(dv["v"]), T,
                                              0.0, ptr(ct), ldc), reps)

    def recon():
        ctx.call("pmd_csr_rows_spmm", ptr(dv["indptr"]), ptr(dv["indices"]), ptr(dv["data"]), ptr(sel), D, ptr(ct), ldc, ldc,
                 ptr(acc), ldc)
        ctx.call("pmd_transpose_affine", ptr(acc), ldc, D, n, ptr(std), None, ptr(W), D)
    out["reconstruction_ms"] = ev_time(recon, reps)
    for name, y in (("fp32", mov_dev), ("i16", mov_dev[:n].to(torch.int16))):   # 16-bit: int16 (same bytes as uint16)
        y2 = y[:n].reshape(n, D).contiguous()
        elem = 0 if name == "fp32" else 2
        ms = ev_time(lambda: ctx.call("pmd_diag_fused_accumulate", ptr(y2), elem, 0, ptr(W), None, 1, 0, n, T, d1, d2,
                                      ptr(mean), ptr(ref), ptr(mom), ptr(fss), ptr(ws), ws.numel()), reps)
        # bytes: the raw frames and the reconstruction once (the eight neighbour loads hit L1 / L2), the fp64 partials
        # written and read back by the block reduction, the moments read and written, the per-frame sums
        nbytes = n * D * (y2.element_size() + 4) + 2 * ws.numel() + 2 * 35 * D * 8
        out["fused_%s_ms" % name] = ms
        out["fused_%s_GB" % name] = nbytes / 1e9
        out["fused_%s_hbm_fraction" % name] = nbytes / (ms * 1e-3) / (HBM_TBS * 1e12)
    pmd.to_host()
    out["block_frames"] = n
    return out


def pinned_rate(dev, nbytes=1 << 30):
    import torch

    h = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    g = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return nbytes / wall(lambda: g.copy_(h, non_blocking=True), 3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--rank", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small-d", type=int, default=128)
    ap.add_argument("--small-T", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import localmd_amd
    from localmd_amd._lib import Context
    from localmd_amd import decomposition as Dm
    from localmd_amd import diagnostic_images as DI

    Dm.QUIET = True
    ctx = Context(0)
    dev = ctx.device
    rec = {"shape": [args.T, args.d, args.d], "rank": args.rank}
    pmd = synthetic_pmd(args.d, args.T, args.rank)
    rec["n_cols"] = int(pmd.u.shape[1])
    mov_dev = movie(args.d, args.T, dev)
    rec.update(phases(ctx, pmd, mov_dev, args.reps))
    frames = args.T
    t = wall(lambda: localmd_amd.make_pmd_diagnostic_images(mov_dev, pmd, ctx=ctx), 1)
    rec["device_tensor_s"] = t
    rec["device_tensor_frames_per_s"] = frames / t
    mov_host = mov_dev.cpu().numpy()
    del mov_dev
    torch.cuda.empty_cache()
    rec["pinned_h2d_GBs"] = pinned_rate(dev)
    for name, src in (("host_fp32", mov_host), ("host_u16", None)):
        if src is None:
            src = mov_host.astype(np.uint16)
        t = wall(lambda: localmd_amd.make_pmd_diagnostic_images(src, pmd, ctx=ctx), 1)
        rate = src.nbytes / t / 1e9
        rec[name + "_s"] = t
        rec[name + "_GBs"] = rate
        rec[name + "_fraction_of_pinned"] = rate / rec["pinned_h2d_GBs"]
        rec[name + "_frames_per_s"] = frames / t
        del src
    del mov_host

    # against the four existing routines on a to_device() PMDArray, at a shape where those finish in reasonable time
    sd, sT = args.small_d, args.small_T
    spmd = synthetic_pmd(sd, sT, min(args.rank, 500), seed=2)
    smov = movie(sd, sT, dev).cpu().numpy()
    spmd.to_device(ctx=ctx)

    def four():
        DI.make_correlation_image(smov, ctx=ctx)
        DI.make_autocorrelation_image(smov, lag=1, ctx=ctx)
        DI.make_pmd_correlation_image(smov, spmd, ctx=ctx)
        DI.make_residual_correlation_image(smov, spmd, ctx=ctx)
    t4 = wall(four, 1)
    t1 = wall(lambda: localmd_amd.make_pmd_diagnostic_images(smov, spmd), args.reps)
    spmd.to_host()
    rec["small_shape"] = [sT, sd, sd]
    rec["small_four_routines_s"] = t4
    rec["small_one_pass_s"] = t1
    rec["small_speedup"] = t4 / t1
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
