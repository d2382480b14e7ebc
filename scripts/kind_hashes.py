"""
A sha256 of every output array of the five per-pixel consumers of a decomposition (summary_images, quantile_images,
regressor_maps, superpixels, rolling_baseline) on one seeded uint16 movie of 2500 x 40 x 44, at frame_batch_size 1024
and 2048: the table two trees are compared by when a change may not move a bit.

The decomposition is run once and its factors are saved to --factors (an .npz); a run that finds the file reads the
factors from it and decomposes nothing, so two trees that read the same file start from the same bits.

    python scripts/kind_hashes.py --factors FILE.npz [--out FILE.txt]
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import scipy.sparse

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, D1, D2 = 2500, 40, 44


def movie():
    from localmd_amd.synthetic import make_movie

    return np.rint(8.0 * make_movie(T, D1, D2, seed=11)).astype(np.float32)


def factors(path, ctx, mov):
    import localmd_amd
    from localmd_amd.pmdarray import PMDArray

    if not os.path.exists(path):
        np.random.seed(0)
        pmd = localmd_amd.localmd_decomposition(mov, (20, 20), 1000, max_components=4, background_rank=1, seed=3,
                                                sim_iters=5, order="F", ctx=ctx)
        u = pmd.u.tocoo()
        np.savez(path, row=u.row, col=u.col, data=u.data, u_shape=np.asarray(u.shape), r=pmd.r, s=pmd.s, v=pmd.v,
                 mean=np.asarray(pmd.mean_img), std=np.asarray(pmd.var_img))
    f = np.load(path)
    u = scipy.sparse.coo_matrix((f["data"], (f["row"], f["col"])), shape=tuple(int(x) for x in f["u_shape"]))
    return PMDArray(u, f["r"], f["s"], f["v"], (T, D1, D2), "F", f["mean"], f["std"])


def outputs(pmd, u16, ctx, fbs):
    """[(name, array)] of every consumer at frame_batch_size ``fbs``."""
    import localmd_amd
    from localmd_amd.summary import STATS

    kw = dict(frame_batch_size=fbs, ctx=ctx)
    kinds = ("denoised", "raw", "residual")
    out = []
    s = localmd_amd.summary_images(pmd, u16, kinds=kinds, stats=STATS, **kw)
    out += [("summary.{}.{}".format(k, st), getattr(s, k)[st]) for k in kinds for st in STATS]
    q = localmd_amd.quantile_images(pmd, u16, kinds=kinds, q=(0.1, 0.5), mad=True, **kw)
    out += [("quantile.{}".format(k), getattr(q, k)) for k in kinds]
    out += [("quantile.mad.{}".format(k), q.mad[k]) for k in kinds]
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, T))
    for stat in ("sum", "correlation"):
        m = localmd_amd.regressor_maps(pmd, x, u16, kinds=kinds, stat=stat, **kw)
        out += [("maps.{}.{}".format(stat, k), getattr(m, k)) for k in kinds]
    for kind in ("denoised", "raw"):
        sp = localmd_amd.superpixels(pmd, u16, kind=kind, **kw)
        out += [("superpixels.{}.{}".format(kind, a), getattr(sp, a))
                for a in ("labels", "sizes", "correlation", "threshold", "edges")]
        for method in ("maximin", "percentile"):
            b = localmd_amd.rolling_baseline(pmd, u16, kind=kind, window=300, method=method, **kw)
            out.append(("baseline.{}.{}".format(kind, method), b.knots))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factors", required=True)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from localmd_amd import decomposition as Dm
    from localmd_amd._lib import Context

    Dm.QUIET = True
    ctx = Context(0)
    mov = movie()
    pmd = factors(args.factors, ctx, mov)
    lines = []
    for fbs in (1024, 2048):
        for name, a in outputs(pmd, mov.astype(np.uint16), ctx, fbs):
            a = np.ascontiguousarray(a)
            lines.append("{}  fbs={} {} {} {}".format(hashlib.sha256(a.tobytes()).hexdigest(), fbs, name, a.dtype,
                                                       a.shape))
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
