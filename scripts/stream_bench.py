"""
Streamed decomposition (stream=True) throughput: pass 1 (statistics + gathers) and pass 2 (projection) in GB/s of
source bytes, frames/s for a fp32 NumPy movie and a uint16 lazy_data_loader, the resident path on the same fp32 movie,
and the staging ring's host-to-device rate per dtype (the bound of both passes).  Prints one JSON line.

    python scripts/stream_bench.py [--d 512] [--T 40000] [--frame-range 5000] [--out profiles/r04_stream_x.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make(T, d, seed=0):
    """Rank-8 Gaussian-blob movie plus a bank of 64 noise frames (fast to build at tens of GB)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:d, 0:d]
    cy, cx = rng.uniform(0, d, 8), rng.uniform(0, d, 8)
    space = np.stack([np.exp(-((yy - a) ** 2 + (xx - b) ** 2) / (d / 4.0)).reshape(-1) for a, b in zip(cy, cx)]).astype(np.float32)
    freq = rng.uniform(0.001, 0.02, 8)
    noise = rng.normal(0, 8.0, (64, d * d)).astype(np.float32)
    mov = np.empty((T, d, d), dtype=np.float32)
    for t0 in range(0, T, 1000):
        idx = np.arange(t0, min(T, t0 + 1000))
        tr = (400.0 * (1.0 + np.sin(idx[:, None] * freq[None, :] * 2 * np.pi))).astype(np.float32)
        fr = tr @ space + 1000.0 + noise[(idx * 7919) % 64]
        mov[t0:t0 + len(idx)] = np.round(fr).reshape(len(idx), d, d)
    return mov


def h2d_rate(dtype, D, step_bytes=64 << 20, reps=20):
    """Pinned staging buffer -> device, GB/s (the copy the streamed passes issue per staging piece)."""
    import torch

    n = max(1, step_bytes // (D * np.dtype(dtype).itemsize))
    tdt = torch.from_numpy(np.zeros(1, dtype=dtype)).dtype
    src = torch.empty((n, D), dtype=tdt, pin_memory=True)
    dst = torch.empty((n, D), dtype=tdt, device="cuda")
    dst.copy_(src, non_blocking=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        dst.copy_(src, non_blocking=True)
    torch.cuda.synchronize()
    return reps * src.numel() * src.element_size() / (time.perf_counter() - t0) / 1e9


def run(src, frame_range, stream, ctx, **kw):
    import localmd_amd

    np.random.seed(1)
    t0 = time.perf_counter()
    _, diag = localmd_amd.localmd_decomposition(src, (20, 20), frame_range, max_components=8, background_rank=15, seed=3,
                                                sim_iters=50, return_diagnostics=True, ctx=ctx, stream=stream, **kw)
    return time.perf_counter() - t0, diag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--T", type=int, default=40000)
    ap.add_argument("--frame-range", type=int, default=5000)
    ap.add_argument("--workers", type=int, default=16, help="reader threads for the lazy_data_loader run")
    ap.add_argument("--skip-resident", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from localmd_amd import decomposition as Dm
    from localmd_amd._movie import _stream_batch_frames
    from localmd_amd._lib import Context
    from localmd_amd.dataset import ArrayDataset

    Dm.QUIET = True
    d, T, D = a.d, a.T, a.d * a.d
    avail = os.sysconf("SC_AVPHYS_PAGES") * os.sysconf("SC_PAGE_SIZE")
    if 7.0 * T * D > 0.8 * avail:    # fp32 movie + its uint16 copy (+ slack) must fit in host memory
        T = max(4096, int(0.8 * avail / (7.0 * D)) // 1024 * 1024)
        print("host memory: T reduced to {}".format(T), file=sys.stderr)
    ctx = Context(0)
    res = {"shape": [T, d, d], "frame_range": a.frame_range, "batch_frames": _stream_batch_frames(10000),
           "h2d_pinned_gbs": {"float32": h2d_rate(np.float32, D), "uint16": h2d_rate(np.uint16, D)}}
    t0 = time.perf_counter()
    mov = make(T, d)
    res["host_generate_s"] = time.perf_counter() - t0
    # warm-up: page-locks the staging rings (kept between calls) and loads every kernel
    run(mov[:4096], 2000, True, ctx)
    run(ArrayDataset(mov[:4096].astype(np.uint16)), 2000, True, ctx, num_workers=a.workers)

    def record(name, wall, diag, src_bytes):
        tm = diag["timings"]
        r = {"wall_s": wall, "frames_per_s": T / wall, "streamed": diag["streamed"],
             "timings_s": {k: round(v, 4) for k, v in tm.items()}}
        if diag["streamed"]:
            r["pass1_gbs"] = src_bytes / tm["stream_stats"] / 1e9
            r["pass2_gbs"] = src_bytes / tm["stream_projection"] / 1e9
            r["bytes_uploaded"] = diag["stream_bytes_uploaded"]
        res[name] = r

    wall, diag = run(mov, a.frame_range, True, ctx)
    record("stream_fp32_numpy", wall, diag, 4 * T * D)
    torch.cuda.empty_cache()
    ctx.release_workspace()
    if not a.skip_resident:
        wall, diag = run(mov, a.frame_range, False, ctx)
        record("resident_fp32_numpy", wall, diag, 4 * T * D)
        torch.cuda.empty_cache()
        ctx.release_workspace()
    mov16 = mov.astype(np.uint16)
    del mov
    wall, diag = run(ArrayDataset(mov16), a.frame_range, True, ctx, num_workers=a.workers)
    record("stream_u16_lazy_loader", wall, diag, 2 * T * D)
    for k, dt in (("stream_fp32_numpy", "float32"), ("stream_u16_lazy_loader", "uint16")):
        h = res["h2d_pinned_gbs"][dt]
        res[k]["pass1_vs_h2d"] = res[k]["pass1_gbs"] / h
        res[k]["pass2_vs_h2d"] = res[k]["pass2_gbs"] / h
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
