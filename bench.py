#!/usr/bin/env python3
"""
Headline benchmark: frames/sec of the full PMD decomposition (BASELINE.json metric) on a
synthetic 512x512x10000 fp32 movie, 20x20 blocks, reference-default arguments, movie resident
in HBM when the clock starts, results (CSR U, R, s, Vt, mean, std) on the host when it stops.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config NAME] [--dump-outputs DIR]
                    [--full [--no-cpu-baseline] [--no-host-input]]

One "step" = one complete decomposition.  Rank 0 prints ONE JSON line carrying the metric.  A plain run does only what
that needs: set-up, warm-up, the timed steps, the dump if asked for, the line.
--dump-outputs DIR writes the PMDArray of the last timed step as DIR/<name>.npy (see dump_outputs).
--full adds, after the timed steps and outside them: one instrumented step (per-phase and per-kernel times, tile
statistics, `roofline` / `roofline_mfma` of the two dominant hand-written kernels, timed with HIP events on their stream),
the same decomposition handed a host array (`frames_per_s_from_host_array`, N=1 only) and `cpu_baseline` (the CPU oracle
timed on a bounded crop of the same movie, rank 0, N=1 only).
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

CONFIGS = {
    # name: (T, d1, d2, block, max_components)
    "demo_60x80x2000": dict(T=2000, d1=60, d2=80, block=20, frames=100, max_components=50),
    "256x256x2000_b20_r8": dict(T=2000, d1=256, d2=256, block=20, frames=2000, max_components=8),
    "512x512x10000_b20": dict(T=10000, d1=512, d2=512, block=20, frames=10000, max_components=50),
    # spatial size / block of BASELINE config 4 with a time axis that fits one GPU next to its working copies
    "1024x1024x2000_b32": dict(T=2000, d1=1024, d2=1024, block=32, frames=2000, max_components=50),
    # the same with a longer time axis (33.5 GB movie: element counts beyond 2^31 in every movie-sized array)
    "1024x1024x8000_b32": dict(T=8000, d1=1024, d2=1024, block=32, frames=8000, max_components=50),
    # block / overlap of BASELINE config 5 on a quarter of its field of view
    "1024x1024x1000_b16": dict(T=1000, d1=1024, d2=1024, block=16, frames=1000, max_components=50),
    # BASELINE configs 4 and 5 at full size (84 GB movies) on ONE GPU: the single-copy memory plan and the tile batches
    # of localmd_decomposition keep them inside 288 GB (BASELINE.json quotes them on 8 GPUs; no such node was available)
    "1024x1024x20000_b32": dict(T=20000, d1=1024, d2=1024, block=32, frames=20000, max_components=50),
    # (config 5: the movie is handed over through a one-shot source, so that localmd_decomposition can release the raw
    # copy once it is standardised - one step only, the movie would have to be rebuilt for a second one)
    "2048x2048x5000_b16": dict(T=5000, d1=2048, d2=2048, block=16, frames=5000, max_components=50, one_shot=True),
}
DEFAULT_CONFIG = "512x512x10000_b20"
FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X dense f32 matrix peak
HBM_PEAK_GBS = 8000.0
DUMP_ARRAY_BYTES = 6 << 20     # per dumped array; the dozen arrays of dump_outputs stay below DUMP_TOTAL_BYTES
DUMP_TOTAL_BYTES = 64 << 20
DUMP_FRAMES = 8
DUMP_U_ENTRIES = 1 << 18


def _sample_rows(name, a):
    """``a`` whole if it fits DUMP_ARRAY_BYTES, else a fixed sample of its rows (axis 0, ascending; the generator is seeded
    by ``name`` only, so equal shapes give equal samples) and the indices of those rows."""
    if a.nbytes <= DUMP_ARRAY_BYTES:
        return a, None
    k = max(1, DUMP_ARRAY_BYTES // (a.nbytes // a.shape[0]))
    idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(a.shape[0], size=k, replace=False))
    return a[idx], idx


def _frames(pmd, fidx):
    """pmd[fidx] (the frames a caller reads back), accumulated in float64.  PMDArray.__getitem__ on the host would form
    (R s) Vt for all frames first; this takes only the selected columns of Vt."""
    vs = pmd.v[:, fidx].astype(np.float64) * pmd.s.astype(np.float64)[:, None]
    temporal = np.empty((pmd.r.shape[0], len(fidx)))
    for i in range(0, pmd.r.shape[0], 4096):
        temporal[i:i + 4096] = pmd.r[i:i + 4096].astype(np.float64) @ vs
    img = (pmd.u @ temporal)[pmd.row_indices]                      # (d1, d2, frames), pixel order of the PMDArray
    img = img * pmd.var_img[..., None].astype(np.float64) + pmd.mean_img[..., None].astype(np.float64)
    return np.ascontiguousarray(np.moveaxis(img, -1, 0), dtype=np.float32)


def dump_outputs(pmd, out_dir):
    """Writes what a caller of the timed path receives - the PMDArray (U as CSR, R, s, Vt, mean and noise images) and
    frames expanded from it - as out_dir/<name>.npy, float32 (values) or float64 (indices and counts).  Arrays larger
    than DUMP_ARRAY_BYTES are replaced by a fixed sample of their rows, with the row indices next to them
    (<name>_rows.npy); U by its per-row entry counts and a fixed sample of its stored entries.  Returns the bytes written."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {}

    def put(name, a, float_dtype=np.float32):
        a, idx = _sample_rows(name, np.ascontiguousarray(a, dtype=float_dtype))
        arrays[name] = a
        if idx is not None:
            arrays[name + "_rows"] = idx.astype(np.float64)

    u = pmd.u
    put("s", pmd.s)
    put("mean_img", pmd.mean_img)
    put("var_img", pmd.var_img)   # the noise std image, under the PMDArray attribute name
    put("u_row_nnz", np.diff(u.indptr), np.float64)
    pos = np.arange(u.nnz)
    if u.nnz > DUMP_U_ENTRIES:
        pos = np.sort(np.random.default_rng(zlib.crc32(b"u_entries")).choice(u.nnz, size=DUMP_U_ENTRIES, replace=False))
    arrays["u_entry_row"] = (np.searchsorted(u.indptr, pos, side="right") - 1).astype(np.float64)
    arrays["u_entry_col"] = u.indices[pos].astype(np.float64)
    arrays["u_entry_value"] = u.data[pos].astype(np.float32)
    put("r", pmd.r)
    put("v", pmd.v)
    T = pmd.shape[0]
    fidx = np.sort(np.random.default_rng(zlib.crc32(b"frames")).choice(T, size=min(T, DUMP_FRAMES), replace=False))
    arrays["frame_index"] = fidx.astype(np.float64)
    frames, rows = _sample_rows("frames", np.moveaxis(_frames(pmd, fidx), 1, 0))   # sampled along the image rows
    arrays["frames"] = np.ascontiguousarray(np.moveaxis(frames, 0, 1))
    if rows is not None:
        arrays["frames_rows"] = rows.astype(np.float64)
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_TOTAL_BYTES, total
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return total


def cpu_baseline(cfg, movie_dev, seed):
    """The CPU oracle (oracle/pmd_oracle.py = NumPy port of the reference) timed on the host cores of this box, on a
    bounded sample of the same workload, in two parts that are summed:
      (a) everything that scales with the field of view - statistics, background basis, standardise / filter, the
          per-tile decompositions, sparse assembly, the movie projection - by running the oracle end to end on a
          128 x 128-pixel window of the same movie (all frames, same arguments; 5 of the 250 threshold simulations,
          whose cost is scaled back up) and scaling the time by the tile count;
      (b) the global stage at the REAL order of the workload, which the window cannot show (there R < frames): with
          R > frames the reference forms C = M^T (G M), W = M^T Z-like products and R = M X - three products of 2 R m^2
          flops - and two symmetric eigendecompositions of order m = min(R, frames) (decomposition.py:976-999,
          :1089-1099).  One product of each kind of shape and one eigendecomposition are timed at full size with the
          NumPy calls the oracle makes (fp32 arrays; numpy.linalg.eigh) and counted three times / twice.
    Only for the headline-like workloads (R > frames); small workloads run the oracle in full."""
    from oracle import pmd_oracle as O, philox

    try:
        from threadpoolctl import threadpool_info

        threads = max([p.get("num_threads", 1) for p in threadpool_info()] + [1])
    except Exception:
        threads = os.cpu_count() or 1
    T, d1, d2, b = cfg["T"], cfg["d1"], cfg["d2"], cfg["block"]
    n_sim = 5
    kw = dict(max_components=cfg["max_components"], rng=philox.PhiloxSource(seed), sim_iters=n_sim)
    full = d1 * d2 * T <= 256 * 256 * 2000
    crop = (d1, d2) if full else (min(d1, 128), min(d2, 128))
    if hasattr(movie_dev, "cpu"):
        sub = movie_dev[:, :crop[0], :crop[1]].cpu().numpy()
    else:
        # one-shot / slab sources are not subscriptable (and a one-shot source has been consumed): the window is generated
        # again from the same formula, identical to the same pixels of the movie that was decomposed
        import torch
        from localmd_amd.synthetic import make_movie_torch

        sub = make_movie_torch(T, d1, d2, torch.device("cuda", 0), seed=0, rows=(0, crop[0]))[:, :, :crop[1]].cpu().numpy()
    np.random.seed(0)
    t0 = time.perf_counter()
    res = O.localmd_decomposition(sub, (b, b), cfg["frames"], **kw)
    dt_crop = time.perf_counter() - t0
    # the 245 threshold simulations that were skipped: time one more and scale
    t0 = time.perf_counter()
    O.threshold_heuristic([b, b, min(cfg["frames"], T)], philox.PhiloxSource(seed + 1), iters=1)
    dt_sim = (time.perf_counter() - t0) * (250 - n_sim)
    tiles_crop = len(res.diag["tile_ranks"])
    stride = b - b // 2
    tiles_full = (len(range(0, d1 - b, stride)) + 1) * (len(range(0, d2 - b, stride)) + 1) if not full else tiles_crop
    scale = tiles_full / float(tiles_crop)
    total = dt_crop * scale + dt_sim
    note = (f"oracle end to end on a {crop[0]}x{crop[1]}x{T} window of the same movie: {dt_crop:.1f} s for {tiles_crop} tiles, scaled by tile "
            f"count x{scale:.2f}; + the 245 skipped threshold simulations ({dt_sim:.1f} s, one timed)")
    if not full:
        mean_rank = float(np.mean(res.diag["tile_ranks"]))
        R_full = int(mean_rank * tiles_full) + 15
        m = min(R_full, cfg["frames"])
        if R_full > cfg["frames"]:
            rng = np.random.default_rng(0)
            a = rng.standard_normal((m, m), dtype=np.float32)
            a = (a + a.T) * np.float32(0.5)
            t0 = time.perf_counter()
            np.linalg.eigh(a)
            dt_eig = time.perf_counter() - t0
            rows = min(R_full, 8192)           # a row block of the R x m operands; the product time scales with the rows
            Mb = rng.standard_normal((rows, m), dtype=np.float32)
            t0 = time.perf_counter()
            Mb.T @ Mb
            dt_prod = (time.perf_counter() - t0) * (R_full / float(rows))
            total += 2 * dt_eig + 3 * dt_prod
            note += (f"; + the global stage at the real order (R ~ {R_full} > frames): 2 x numpy.linalg.eigh of order {m} ({dt_eig:.1f} s each) + "
                     f"3 x (R x m)^T (R x m) fp32 products ({dt_prod:.1f} s each, timed on {rows} rows)")
    return {"value": T / total, "unit": "frames/s", "cores": int(threads), "kind": "port", "sample": note,
            "cpu_seconds_estimated_full_workload": total}


def rooflines(workload, cfg, diag, prof):
    """The two roofline objects of a --full bench line, from the diagnostics and the per-kernel HIP-event times of the
    instrumented step: (`roofline` = the dominant kernel by time, `roofline_mfma` = tile_atx)."""
    # roofline of the dominant hand-written kernel: tile_atx (four launches per step: V_ds = U_ds^T X,
    # W = U0^T X, the sketch Q^T A and the full-movie projection U^T X).  Algorithmic work per launch
    # (DESIGN.md): flops = 2 * r * d * T per tile with r = max_components (not the padded 64 rows).
    n_tiles = len(diag["tile_ranks"])
    d = cfg["block"] ** 2
    r = diag["max_components"]
    crop = diag["crop"]
    # "tile_atx_main" = the d x T launches only (V_ds, W, and the two projections U^T X of the fit and of the
    # whole movie); the small sketch / simulation / background launches are timed under "tile_atx".
    atx_ms, atx_n = prof.get("tile_atx_main", (0.0, 0))
    flops_per_launch = 2.0 * r * d * crop * n_tiles
    bytes_per_launch = 4.0 * d * crop * n_tiles
    avg_ms = atx_ms / max(atx_n, 1)
    achieved = flops_per_launch / (avg_ms * 1e-3) / 1e12 if avg_ms > 0 else 0.0
    roofline = {
        "kernel": "tile_atx (v_mfma_f32_16x16x4_f32)", "bound": "mfma", "achieved": achieved,
        "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achieved / FP32_MFMA_PEAK_TFLOPS, "traffic": None,
        "avg_launch_ms": avg_ms, "launches_timed": atx_n, "algorithmic_gflop_per_launch": flops_per_launch / 1e9,
        "algorithmic_gb_per_launch": bytes_per_launch / 1e9,
        "hbm_gbs_equiv": bytes_per_launch / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0,
    }
    # HBM-side traffic of the same launch from the committed counter pass; valid for the workload it was taken on and while
    # the kernel source is unchanged (SHA-256 recorded with the pass)
    try:
        import hashlib

        root = os.path.dirname(os.path.abspath(__file__))
        pmc = json.load(open(os.path.join(root, "profiles", "r03_pmc_tile_atx.json")))
        sha = hashlib.sha256(open(os.path.join(root, pmc["kernel_source"]), "rb").read()).hexdigest()
        if workload != DEFAULT_CONFIG:
            roofline["traffic_note"] = "no counter pass for this workload"
        elif sha != pmc["kernel_source_sha256"]:
            roofline["traffic_note"] = "stale: the kernel source changed since the counter pass (profiles/r03_pmc_tile_atx.json)"
        else:
            roofline["traffic"] = pmc["fetch_bytes_per_launch"] / 1e9
            roofline["traffic_unit"] = "GB per launch (L2 -> fabric reads, Infinity Cache hits included)"
            roofline["traffic_source"] = "profiles/r03_pmc_tile_atx.json (separate rocprofv3 --pmc FETCH_SIZE pass, gfx950 x2 correction)"
    except (OSError, KeyError, ValueError):
        roofline["traffic_note"] = "no committed counter pass found"
    roofline_mfma = roofline
    # Dominant kernel by time: sytrd_symv (triangle matrix-vector product of the tridiagonalisation behind the
    # final SVD, one launch per column of the min(R', T)-sized Gram matrix).  Algorithmic bytes per launch =
    # 4 B x the n'(n'+1)/2 entries of the trailing triangle (n' = n - j - 1); with profiling on, the library
    # times every 64th launch (j = 32, 96, ...) on its stream: average bytes / average duration of that sample.
    sv_ms, sv_n = prof.get("sytrd_symv_sample", (0.0, 0))
    n_eig = int(diag["eig_order"])
    if sv_n > 0:
        js = np.arange(32, n_eig - 1, 64, dtype=np.float64)
        npr = n_eig - js - 1
        avg_bytes = float(np.mean(4.0 * npr * (npr + 1) / 2))
        avg_sv_ms = sv_ms / sv_n
        ach = avg_bytes / (avg_sv_ms * 1e-3) / 1e9
        roofline = {
            "kernel": "sytrd_symv (triangle symv of the Householder tridiagonalisation, fp32)", "bound": "hbm",
            "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": None,
            "avg_launch_ms": avg_sv_ms, "launches_timed": sv_n, "launches_per_step": n_eig - 1,
            "algorithmic_mb_per_launch": avg_bytes / 1e6, "matrix_order": n_eig,
        }
        # fabric-side traffic of the same launches from the committed PMC pass (profiles/r03_pmc_sytrd_n10000.json:
        # separate rocprofv3 --pmc FETCH_SIZE run over one n = 10^4 tridiagonalisation, gfx950 x2 correction applied,
        # mean over the launches j = 32, 96, ... that are timed here); only valid for a matrix of that order
        # A counter pass cannot run inside this process (rocprofv3 wraps the program), so the figure is the committed
        # one - valid only for a matrix of that order AND while the kernel's source is the file it was measured on
        # (SHA-256 recorded with the pass); otherwise `traffic` stays null and says why.
        try:
            import hashlib

            root = os.path.dirname(os.path.abspath(__file__))
            pmc = json.load(open(os.path.join(root, "profiles", "r03_pmc_sytrd_n10000.json")))
            sha = hashlib.sha256(open(os.path.join(root, pmc["kernel_source"]), "rb").read()).hexdigest()
            if abs(n_eig - pmc["matrix_order"]) > 1:
                roofline["traffic_note"] = "no counter pass for a matrix of this order"
            elif sha != pmc["kernel_source_sha256"]:
                roofline["traffic_note"] = "stale: the kernel source changed since the counter pass (profiles/r03_pmc_sytrd_n10000.json)"
            else:
                roofline["traffic"] = pmc["traffic_bytes_per_launch_sample_mean"] / 1e9
                roofline["traffic_unit"] = "GB per launch (L2 -> fabric reads, Infinity Cache hits included)"
                roofline["traffic_over_algorithmic"] = pmc["traffic_over_algorithmic_sample"]
                roofline["traffic_source"] = "profiles/r03_pmc_sytrd_n10000.json (separate rocprofv3 --pmc FETCH_SIZE pass, gfx950 x2 correction)"
        except (OSError, KeyError, ValueError):
            roofline["traffic_note"] = "no committed counter pass found"
    return roofline, roofline_mfma


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default=DEFAULT_CONFIG, choices=sorted(CONFIGS))
    ap.add_argument("--full", action="store_true",
                    help="also the instrumented step (phases, kernel times, rooflines), the host-array run and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-host-input", action="store_true", help="with --full: skip the extra run that starts from a host array")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the result of the last timed step as DIR/<name>.npy (at most 64 MB, see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # PMD_BENCH_ONE_DEVICE=1: rehearse the multi-rank path on a one-GPU box (gloo, all ranks on cuda:0)
        if os.environ.get("PMD_BENCH_ONE_DEVICE"):
            local_rank = 0
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")

    import localmd_amd
    from localmd_amd import decomposition as Dm
    from localmd_amd._lib import Context
    from localmd_amd.synthetic import make_movie_torch

    Dm.QUIET = True
    cfg = CONFIGS[args.config]
    device = torch.device("cuda", local_rank)
    if world > 1:
        # every rank builds only the pixel slab of its band of tile rows (same values as the single-GPU movie)
        from localmd_amd.synthetic import SyntheticSlabSource

        movie = SyntheticSlabSource(cfg["T"], cfg["d1"], cfg["d2"], device, seed=0)
    elif cfg.get("one_shot"):
        class OneShotSource:
            """Hands the resident movie over ONCE (slab() drops its own reference): the decomposition then owns the only copy."""

            def __init__(self, tensor):
                self.shape = tuple(tensor.shape)
                self._t = tensor

            def slab(self, i_lo, i_hi):
                t, self._t = self._t, None
                if t is None:
                    raise RuntimeError("one-shot source already consumed")
                return t[:, i_lo:i_hi, :]

        def fresh_movie():
            # the movie is rebuilt (untimed) before every step: the step before consumed the only copy
            return OneShotSource(make_movie_torch(cfg["T"], cfg["d1"], cfg["d2"], device, seed=0))

        if args.no_host_input is False:
            args.no_host_input = True
        movie = None
    else:
        movie = make_movie_torch(cfg["T"], cfg["d1"], cfg["d2"], device, seed=0)
    ctx = Context(local_rank)
    seed = 2024

    def one_step(diag=False):
        np.random.seed(0)
        return localmd_amd.localmd_decomposition(
            movie, (cfg["block"], cfg["block"]), cfg["frames"], max_components=cfg["max_components"], seed=seed,
            ctx=ctx, return_diagnostics=diag, distributed=world > 1)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # The timed steps run WITHOUT the library's HIP-event profiling (round-2 verdict: measurement overhead does not
    # belong in the headline number); with --full, the per-kernel times and both roofline objects come from the one extra,
    # untimed, instrumented step below.  Each step's result is dropped inside the timed region as it always was, except
    # the last one's when --dump-outputs asks for it.
    cold_ms = None
    result = None
    if cfg.get("one_shot"):
        # one-shot workloads (the movie fills a third of the HBM and is consumed by the step): every step gets a freshly
        # built movie, built outside the timed regions; each timed step is bracketed on its own and the times are summed
        for w in range(args.warmup):
            movie = fresh_movie()
            barrier()
            tc = time.perf_counter()
            one_step()
            barrier()
            if w == 0:
                cold_ms = 1e3 * (time.perf_counter() - tc)   # first call of the process: every allocation is new
        elapsed = 0.0
        for i in range(args.steps):
            movie = fresh_movie()
            barrier()
            t0 = time.perf_counter()
            result = one_step()
            if not (args.dump_outputs and i == args.steps - 1):
                result = None
            barrier()
            elapsed += time.perf_counter() - t0
    else:
        for _ in range(args.warmup):
            one_step()
        barrier()
        t0 = time.perf_counter()
        for i in range(args.steps):
            result = one_step()
            if not (args.dump_outputs and i == args.steps - 1):
                result = None
        barrier()
        elapsed = time.perf_counter() - t0
    if cfg.get("one_shot") and movie is not None and getattr(movie, "_t", None) is None:
        movie = None
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    dumped_bytes = None
    if args.dump_outputs and rank == 0:   # the other ranks of the sharded route return None
        dumped_bytes = dump_outputs(result, args.dump_outputs)
    result = None
    ms_per_step = 1e3 * elapsed / args.steps
    # N ranks decompose ONE movie together (tile grid sharded, results gathered): total work is fixed
    value = cfg["T"] * args.steps / elapsed

    out = {
        "metric": "frames/sec PMD decomposition", "value": value, "unit": "frames/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
        "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": args.config, "fov": [cfg["d1"], cfg["d2"]], "frames": cfg["T"], "block": cfg["block"],
                   "frames_to_init": cfg["frames"], "max_components": cfg["max_components"],
                   "parallelism": "1 process per GPU" + (
                       f", bands of tile rows / pixel slabs and the rows of the global stage sharded over {world} ranks "
                       "(tile results gathered, background projection and the two frames x frames Gram matrices "
                       "all-reduced, R collected on rank 0; the m x m Cholesky / eigen stage replicated)" if world > 1 else "")},
        "arithmetic": "fp32 operands, results and accumulation; products of >= 100 GFLOP outside the tile stage run as three "
                      "fp16-piece matrix-core products per product (two fp16 pieces per operand, power-of-two scaling, measured "
                      "error below the sgemm path's: DESIGN 4a, tests/test_gpu_kernels.py::test_gemm_fp16_pieces); M^T G M "
                      "from three exact fp16 pieces per operand (six exact piece products as one matrix product per 2048-term "
                      "accumulation chunk); the Gram matrices and the tile stage are fp32 MFMA; PMD_GEMM_SPLIT=0 = sgemm everywhere",
    }
    if cold_ms is not None:
        out["cold_first_step_ms"] = cold_ms   # the first call of the process (every device / pinned allocation is new)
    if dumped_bytes is not None:
        out["dumped_outputs"] = {"dir": args.dump_outputs, "bytes": dumped_bytes}

    if args.full:
        # one extra, untimed, instrumented run: per-phase breakdown, tile statistics, per-kernel HIP-event times
        if cfg.get("one_shot"):
            movie = fresh_movie()
        ctx.profile_enable(True)
        _, diag = one_step(diag=True)
        barrier()
        prof = ctx.profile_summary()
        ctx.profile_enable(False)
        # PCIe-inclusive figure (never `value`): the same decomposition handed a HOST array (pageable NumPy memory), i.e.
        # including the staging through pinned buffers and the H2D transfer (localmd_amd/decomposition.py: _Movie._stream_in)
        host_rate = None
        if world == 1 and not args.no_host_input and not cfg.get("one_shot"):
            host_movie = movie.cpu().numpy()
            # two runs, the second one timed: the first also page-locks the ring of staging buffers, which the library keeps
            # between calls (0.25 s of a cold 1.19 s at config 3; the steady state of a process that decomposes movie after movie)
            for rep in range(2):
                np.random.seed(0)
                torch.cuda.synchronize()
                th = time.perf_counter()
                localmd_amd.localmd_decomposition(host_movie, (cfg["block"], cfg["block"]), cfg["frames"], max_components=cfg["max_components"],
                                                  seed=seed, ctx=ctx)
                torch.cuda.synchronize()
                host_rate = cfg["T"] / (time.perf_counter() - th)
            del host_movie
        roofline, roofline_mfma = rooflines(args.config, cfg, diag, prof)
        out["config"].update({"tiles": len(diag["tile_ranks"]), "rank_before": diag["rank_before"],
                              "rank_after": diag["rank_after"], "mean_tile_rank": float(np.mean(diag["tile_ranks"]))})
        out.update({
            "roofline": roofline,
            "roofline_mfma": roofline_mfma,
            "frames_per_s_from_host_array": host_rate,
            "phases_ms": {k: 1e3 * v for k, v in diag["timings"].items()},
            "kernel_ms_per_step": {k: v[0] for k, v in sorted(prof.items(), key=lambda kv: -kv[1][0])},
            "kernel_ms_source": "HIP events on the launch stream during one untimed instrumented step",
        })
    out["hbm_peak_allocated_gb"] = torch.cuda.max_memory_allocated(device) / 2 ** 30
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(cfg, movie, seed)
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
