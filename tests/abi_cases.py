"""
Case table of tests/test_gpu_abi_conventions.py: one row per entry point of include/pmd_hip.h that takes a workspace, at the
smallest shapes where its code path still differs, plus the workspace-free calls the stream tests need (pmd_gemm, pmdk_syevd).

A row is a builder ``f(ctx) -> Case``.  A Case owns the device buffers of one call: ``ins`` (what the call reads; some are
also written) with two complete, valid value sets ``A`` and ``B`` for them, ``outs`` (only written), the host integers the
call returns through pointers, and ``run(ctx, ws_ptr, ws_bytes) -> return code``, the call itself through ``ctx.lib`` with
no synchronisation added.  The inputs come from the builders of the existing test modules (_spd, _indefinite, _stats_movie,
_rsvd_input, tile_stage_ref, the residual-window inputs, _eig_mats).

Reproducibility: every row below gave the same bits in two calls on the same workspace fill on an MI355X, so
test_exact_workspace compares bits; a row that should ever stop doing so fails there by name and then needs the fp64
reference of its entry point's own test instead.

CONSUMERS: consumers of a decomposition, section 1 only (their own tests assert their refusals, and the two correlations take
any size from one frame's partials up).  COVERED_ELSEWHERE names the two remaining size functions of the header;
test_table_lists_every_size_function holds rows and pointers against the header.
"""
import ctypes as C
import zlib

import numpy as np

PMD_ERR_WORKSPACE = -3
PREFILL = 0x5A            # every byte of an output array before a call


def _t():
    import torch

    return torch


def P(t):
    return None if t is None else t.data_ptr()


def same_bits(a, b):
    """Two results of Case.bits(): equal byte for byte (NaN patterns included)."""
    torch = _t()
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if isinstance(x, int):
            if x != y:
                return False
        elif x.shape != y.shape or not torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)):
            return False
    return True


class Case:
    def __init__(self, ctx, size_fn, size_args, run, ins, A, B, outs, host=(), compare=None):
        torch = _t()
        self.size_fn = size_fn
        self.nbytes = int(getattr(ctx.lib, size_fn)(*size_args)) if size_fn else 0
        self.run = run
        self.ins, self.outs, self.host = list(ins), list(outs), list(host)
        dev = lambda v: v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)).to(ctx.device)
        self.A, self.B = [dev(v) for v in A], [dev(v) for v in B]
        for t, a, b in zip(self.ins, self.A, self.B):
            assert t.shape == a.shape == b.shape and t.dtype == a.dtype == b.dtype, (t.shape, a.shape, b.shape)
        self.compare = list(outs) if compare is None else list(compare)
        self.reference = None     # bits of the call on inputs A on the session context (test module, first use)

    def load(self, which="A"):
        """Inputs <- value set `which` (enqueued on torch's current stream), every output byte <- PREFILL, host integers <- -1."""
        self.copy_inputs(which)
        for t in self.outs:
            t.view(_t().uint8).fill_(PREFILL)
        for h in self.host:
            h.value = -1

    def copy_inputs(self, which):
        for t, v in zip(self.ins, getattr(self, which)):
            t.copy_(v, non_blocking=True)

    def bits(self):
        return [t.clone() for t in self.compare] + [int(h.value) for h in self.host]

    def untouched(self, which="A"):
        """Outputs still PREFILL, inputs still value set `which`, host integers still -1."""
        torch = _t()
        return (all(bool((t.view(torch.uint8) == PREFILL).all()) for t in self.outs) and
                all(torch.equal(t.view(torch.uint8), v.view(torch.uint8)) for t, v in zip(self.ins, getattr(self, which))) and
                all(h.value == -1 for h in self.host))


def _empty(ctx, shape, dtype=None):
    torch = _t()
    return torch.empty(shape, dtype=dtype or torch.float32, device=ctx.device)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# global stage
def orthogonalize(R, m, has_m):
    def build(ctx):
        from tests.test_gpu_global_stage import _indefinite

        ldm, ldp = m + 3, m + 2
        sets = []
        for s in "AB":
            rng = _rng("orth", R, m, has_m, s)
            sets.append([_indefinite(rng, R)[0]] + ([_f32(rng.standard_normal((R, ldm)))] if has_m else []))
        G, Pm, rp = _empty(ctx, (R, R)), _empty(ctx, (R, ldp)), C.c_int(-1)
        M = _empty(ctx, (R, ldm)) if has_m else None

        def run(cx, ws, nb):
            return cx.lib.pmd_orthogonalize(cx.handle, P(G), R, P(M), m, ldm if has_m else 0, P(Pm), ldp, C.byref(rp), ws, nb)

        return Case(ctx, "pmd_orthogonalize_workspace_bytes", (R, m, int(has_m)), run, [G, M] if has_m else [G], sets[0],
                    sets[1], [Pm], [rp])

    return build


def orthogonalize_factored(Rc, m):
    def build(ctx):
        from tests.test_gpu_global_stage import _indefinite

        sets = []
        for s in "AB":
            rng = _rng("orthf", Rc, m, s)
            Mh = _f32(rng.standard_normal((Rc, m)))
            sets.append([Mh, _f32(_indefinite(rng, Rc)[0].astype(np.float64) @ Mh)])
        M, GM, Et, rp = _empty(ctx, (Rc, m)), _empty(ctx, (Rc, m)), _empty(ctx, (m, m)), C.c_int(-1)

        def run(cx, ws, nb):
            return cx.lib.pmd_orthogonalize_factored(cx.handle, P(M), Rc, m, m, P(GM), m, P(Et), m, C.byref(rp), ws, nb)

        return Case(ctx, "pmd_orthogonalize_factored_workspace_bytes", (m,), run, [M, GM], sets[0], sets[1], [Et], [rp])

    return build


def _m_gm(tag, rows, m, ldm, ldgm):
    sets = []
    for s in "AB":
        rng = _rng(tag, rows, m, s)
        Mh = _f32(rng.standard_normal((rows, ldm)))
        GMh = _f32(rng.standard_normal((rows, ldgm)) * 0.5)
        GMh[:, :m] += Mh[:, :m]
        sets.append([Mh, GMh])
    return sets


def gram_mtgm(rows, m):
    def build(ctx):
        ldm, ldgm, ldc = m + 3, m + 5, m + 2
        sets = _m_gm("mtgm", rows, m, ldm, ldgm)
        M, GM, Cm = _empty(ctx, (rows, ldm)), _empty(ctx, (rows, ldgm)), _empty(ctx, (m, ldc))

        def run(cx, ws, nb):
            return cx.lib.pmd_gram_mtgm(cx.handle, P(M), rows, m, ldm, P(GM), ldgm, P(Cm), ldc, ws, nb)

        return Case(ctx, "pmd_gram_mtgm_workspace_bytes", (rows, m), run, [M, GM], sets[0], sets[1], [Cm])

    return build


def chol_inverse(m, abs_last):
    def build(ctx):
        from tests.test_gpu_global_stage import _spd

        sets = []
        for s in "AB":
            S = _spd(_rng("chol", m, s), m, 1e2) * (1.0 if s == "A" else 2.5)     # (order 1: _spd is [[1]])
            buf = np.full((m, m + 1), 7.0, dtype=np.float32)
            buf[:, :m] = ((S + S.T) / 2).astype(np.float32)
            sets.append([buf])
        Cd, ok = _empty(ctx, (m, m + 1)), C.c_int(-1)

        def run(cx, ws, nb):
            return cx.lib.pmd_chol_inverse(cx.handle, P(Cd), m, m + 1, abs_last, C.byref(ok), ws, nb)

        return Case(ctx, "pmd_chol_inverse_workspace_bytes", (m,), run, [Cd], sets[0], sets[1], [], [ok], compare=[Cd])

    return build


def orthogonalize_chol(Rc, m):
    def build(ctx):
        sets = []
        for s in "AB":
            Mh = _f32(_rng("ochol", Rc, m, s).standard_normal((Rc, m)))
            sets.append([Mh, Mh.copy()])       # G = I: C = M^T M, positive definite
        M, GM, Et, ok = _empty(ctx, (Rc, m)), _empty(ctx, (Rc, m)), _empty(ctx, (m, m)), C.c_int(-1)

        def run(cx, ws, nb):
            return cx.lib.pmd_orthogonalize_chol(cx.handle, P(M), Rc, m, m, P(GM), m, P(Et), m, C.byref(ok), ws, nb)

        return Case(ctx, "pmd_orthogonalize_chol_workspace_bytes", (Rc, m), run, [M, GM], sets[0], sets[1], [Et], [ok])

    return build


def projected_svd(rows_p, n1, n2, with_p=True):
    def build(ctx):
        nk = min(n1, n2)
        ldp, ldv, ldr, ldvt = n1 + 2, n2 + 1, nk + 5, n2 + 3
        rr = rows_p if with_p else n1
        sets = []
        for s in "AB":
            rng = _rng("psvd", rows_p, n1, n2, with_p, s)
            sets.append([_f32(rng.standard_normal((n1, ldv)) * np.logspace(0, -2, ldv)[None, :])] +
                        ([_f32(rng.standard_normal((rows_p, ldp)))] if with_p else []))
        V, Pm = _empty(ctx, (n1, ldv)), (_empty(ctx, (rows_p, ldp)) if with_p else None)
        R, s_, Vt = _empty(ctx, (rr, ldr)), _empty(ctx, (nk,)), _empty(ctx, (nk, ldvt))

        def run(cx, ws, nb):
            return cx.lib.pmd_projected_svd(cx.handle, P(Pm), rows_p if with_p else 0, ldp if with_p else 0, P(V), n1, n2, ldv,
                                            P(R), ldr, P(s_), P(Vt), ldvt, ws, nb)

        return Case(ctx, "pmd_projected_svd_workspace_bytes", (rows_p if with_p else 0, n1, n2), run, [V, Pm] if with_p else [V],
                    sets[0], sets[1], [R, s_, Vt])

    return build


def psvd_finish(rp, nc):
    def build(ctx):
        ldc, ncs = (rp + 3) // 4 * 4, max(nc, 1)
        sets = []
        for s in "AB":
            rng = _rng("finish", rp, nc, s)
            Vp = rng.standard_normal((rp, ncs)) * np.logspace(0, -2, rp)[:, None]
            G = Vp @ Vp.T if nc else (lambda X: X @ X.T)(rng.standard_normal((rp, rp + 5)))
            Cm = np.zeros((rp, ldc), dtype=np.float32)
            Cm[:, :rp] = G
            sets.append([Cm, _f32(Vp)])
        Cd, Vpd = _empty(ctx, (rp, ldc)), _empty(ctx, (rp, ncs))
        W, s_, Vt = _empty(ctx, (rp, rp)), _empty(ctx, (rp,)), _empty(ctx, (rp, ncs))

        def run(cx, ws, nb):
            return cx.lib.pmd_psvd_finish(cx.handle, P(Cd), ldc, rp, P(Vpd), nc, ncs, P(W), rp, P(s_), P(Vt), ncs, ws, nb)

        return Case(ctx, "pmd_psvd_finish_workspace_bytes", (rp,), run, [Cd, Vpd], sets[0], sets[1], [W, s_, Vt])

    return build


def projected_svd_factored(Rc, m, rp, T):
    def build(ctx):
        sets = []
        for s in "AB":
            rng = _rng("psvdf", Rc, m, rp, T, s)
            Et = rng.standard_normal((rp, m)) * 0.05
            Et[:, :rp] += np.eye(rp)
            sets.append([_f32(rng.standard_normal((Rc, m))), _f32(Et),
                         _f32(rng.standard_normal((Rc, T)) * np.logspace(0, -2, T)[None, :])])
        M, Et, Z = _empty(ctx, (Rc, m)), _empty(ctx, (rp, m)), _empty(ctx, (Rc, T))
        R, s_, Vt = _empty(ctx, (Rc, rp)), _empty(ctx, (rp,)), _empty(ctx, (rp, T))

        def run(cx, ws, nb):
            return cx.lib.pmd_projected_svd_factored(cx.handle, P(M), Rc, m, m, P(Et), rp, m, P(Z), T, T, P(R), rp, P(s_), P(Vt), T,
                                                     None, 0, None, None, 0, ws, nb)

        return Case(ctx, "pmd_projected_svd_factored_workspace_bytes", (Rc, m, rp, T), run, [M, Et, Z], sets[0], sets[1],
                    [R, s_, Vt])

    return build


# ---------------------------------------------------------------------------------------------------------------------
# movie preparation (the smallest parametrisations of test_gpu_prep_stage.py; pmd_stats at 256 frames, the fewest that
# enter the Welch estimate and so use the second workspace array)
STATS_T, STATS_D = 256, 117


def _stats_sets():
    from tests.test_gpu_prep_stage import _stats_movie

    return [[_stats_movie("plain", STATS_T, STATS_D).copy()], [_stats_movie("camera", STATS_T, STATS_D).copy()]]


def stats(ctx):
    T, D = STATS_T, STATS_D
    sets = _stats_sets()
    mov, mean, std = _empty(ctx, (T, D)), _empty(ctx, (D,)), _empty(ctx, (D,))

    def run(cx, ws, nb):
        return cx.lib.pmd_stats(cx.handle, P(mov), T, D, 1024, 1, P(mean), P(std), ws, nb)

    return Case(ctx, "pmd_stats_workspace_bytes", (T, D, 1024), run, [mov], sets[0], sets[1], [mean, std])


def stats_stream(ctx):
    """accumulate (the whole movie as one fp32 batch) + finish on one workspace, as the streamed statistics pass runs them."""
    T, D = STATS_T, STATS_D
    sets = _stats_sets()
    mov, mean, std = _empty(ctx, (T, D)), _empty(ctx, (D,)), _empty(ctx, (D,))

    def run(cx, ws, nb):
        rc = cx.lib.pmd_stats_stream_accumulate(cx.handle, P(mov), 0, 0, T, T, D, 1, ws, nb)
        return rc if rc else cx.lib.pmd_stats_stream_finish(cx.handle, T, D, 1, P(mean), P(std), ws, nb)

    return Case(ctx, "pmd_stats_stream_workspace_bytes", (T, D), run, [mov], sets[0], sets[1], [mean, std])


def bg_project(ctx):
    from tests.test_gpu_prep_stage import _orthonormal

    D, T, K = 360, 120, 3
    ld = int(ctx.lib.pmd_time_ld(T)) + 64
    ldp = ld + 32
    sets = []
    for s in "AB":
        rng = _rng("bgp", s)
        x = np.zeros((1024, ld), dtype=np.float32)
        x[:D, :T] = rng.standard_normal((D, T))
        sets.append([x, _orthonormal(rng, D, K)])
    xs, basis, pj = _empty(ctx, (1024, ld)), _empty(ctx, (D, K)), _empty(ctx, (K, ldp))

    def run(cx, ws, nb):
        return cx.lib.pmd_bg_project(cx.handle, P(xs), D, T, ld, P(basis), K, P(pj), ldp, ws, nb)

    return Case(ctx, "pmd_bg_project_workspace_bytes", (D, T), run, [xs, basis], sets[0], sets[1], [pj])


def background_rsvd(ctx):
    from tests.test_gpu_prep_stage import RSVD_SEED, _rsvd_input

    D, n, K = 100, 80, 4
    ld = int(ctx.lib.pmd_time_ld(n))
    sets = []
    for ratio in (0.7, 0.8):
        x = np.zeros((1024, ld), dtype=np.float32)
        x[:D, :n] = _rsvd_input(D, n, K, ratio)
        sets.append([x])
    xs, basis = _empty(ctx, (1024, ld)), _empty(ctx, (D, K))

    def run(cx, ws, nb):
        return cx.lib.pmd_background_rsvd(cx.handle, P(xs), D, n, ld, K, RSVD_SEED, P(basis), ws, nb)

    return Case(ctx, "pmd_background_rsvd_workspace_bytes", (D, n, K), run, [xs], sets[0], sets[1], [basis])


def threshold_sim(ctx):
    """No device input: the seed is the input (the stream test of this row checks that nothing is written early)."""
    from tests.test_gpu_prep_stage import SIM_SEED

    b1, b2, t, iters = 10, 12, 64, 8
    out = _empty(ctx, (iters, 2))

    def run(cx, ws, nb):
        return cx.lib.pmd_threshold_sim(cx.handle, b1, b2, t, iters, SIM_SEED, P(out), ws, nb)

    return Case(ctx, "pmd_threshold_sim_workspace_bytes", (b1, b2, t, iters), run, [], [], [], [out])


# ---------------------------------------------------------------------------------------------------------------------
# tile stage
def tiles_decompose(ctx):
    """Case F1n of tile_stage_ref (four 20 x 20 tiles of a 30 x 30 x 100 movie, r = 20), the arguments of its device_run."""
    from localmd_amd import grid
    from tests import tile_stage_ref as R

    torch, lib, name = _t(), ctx.lib, "F1n"
    c = R.cfg(name)
    (d1, d2), (b1, b2), T = R.case_dims(name)
    a, r, D, d = c["a"], c["r"], d1 * d2, b1 * b2
    pix_all, _ = R.tiles(name)
    n = len(pix_all)
    pool_q, pool_idx, pool_w, _ = grid.pooling_maps((b1, b2), c["pool"])
    Pn = pool_q.shape[0]
    rp, dpad, ld = int(lib.pmd_tile_rpad(r)), int(lib.pmd_tile_dpad(d)), int(lib.pmd_time_ld(T))
    rows = R.movie_rows(name)
    sets = []
    for mov in (rows, rows[::-1, ::-1] * np.float32(-0.5)):
        x = np.zeros((D, ld), dtype=np.float32)
        x[:, :T] = mov
        sets.append([x])
    xf = _empty(ctx, (D, ld))
    ut, v, st = _empty(ctx, (n, rp, dpad)), _empty(ctx, (n, rp, ld)), _empty(ctx, (n, rp, 2))
    good, keep, ranks = _empty(ctx, (n, rp), torch.int32), _empty(ctx, (n, rp), torch.int32), _empty(ctx, (n,), torch.int32)
    lam = _empty(ctx, (n, rp), torch.float64)
    tabs = [R.to_device(ctx, pix_all, np.int32), R.to_device(ctx, pool_q, np.int32), R.to_device(ctx, pool_idx, np.int32),
            R.to_device(ctx, pool_w, np.float32)]
    i0, step = R.omega_indices(name)
    thr = c["thr"]

    def run(cx, ws, nb):
        return cx.lib.pmd_tiles_decompose(cx.handle, P(xf), ld, D, T, P(tabs[0]), n, b1, b2, P(tabs[1]), pool_q.shape[1], Pn,
                                          P(tabs[2]), P(tabs[3]), r, a, float(thr[0]), float(thr[1]), 2, R.SEED, i0, step, P(ut),
                                          P(v), ld, P(st), P(good), P(keep), P(ranks), P(lam), ws, nb)

    return Case(ctx, "pmd_tiles_workspace_bytes", (n, b1, b2, Pn, r, a, T, ld, D), run, [xf], sets[0], sets[1],
                [ut, v, st, good, keep, ranks, lam])


def tiles_residual(ctx):
    """Case B of test_gpu_residual_window (four 16 x 24 tiles, a 300-frame window, r = 6), the arguments of its _call."""
    from tests import test_gpu_residual_window as W

    torch, lib, name = _t(), ctx.lib, "B"
    c, inp = W.CASES[name], W._inputs(name)
    (b1, b2), L, a, r, bases = c["block"], c["L"], c["a"], c["r"], c["bases"]
    n, d, D = len(bases), b1 * b2, inp["X"].shape[0]
    rp, dpad, ld = int(lib.pmd_tile_rpad(r)), int(lib.pmd_tile_dpad(d)), int(lib.pmd_time_ld(L))
    u0 = np.zeros((n, rp, dpad), dtype=np.float32)
    for t in range(n):
        u0[t, :bases[t], :d] = inp["E"][t].T
    sets = []
    for mov in (inp["X"], inp["X"][::-1, ::-1] * np.float32(-0.5)):
        x = np.zeros((D, ld), dtype=np.float32)
        x[:, :L] = mov
        sets.append([x, u0.copy(), np.asarray(bases, dtype=np.int32)])
    xw, ucur, counts = _empty(ctx, (D, ld)), _empty(ctx, (n, rp, dpad)), _empty(ctx, (n,), torch.int32)
    st, good, keep = _empty(ctx, (n, rp, 2)), _empty(ctx, (n, rp), torch.int32), _empty(ctx, (n, rp), torch.int32)
    pix = torch.from_numpy(np.ascontiguousarray(inp["pix"], dtype=np.int32)).to(ctx.device)
    i0, step = W._omega_indices(name)
    thr = W._thresholds(name)[0]

    def run(cx, ws, nb):
        return cx.lib.pmd_tiles_residual(cx.handle, P(xw), ld, D, L, P(pix), n, b1, b2, r, a, thr[0], thr[1], 2, W.SEED, i0, step,
                                         P(ucur), P(counts), P(st), P(good), P(keep), ws, nb)

    return Case(ctx, "pmd_tiles_residual_workspace_bytes", (n, b1, b2, r, a, L, D), run, [xw, ucur, counts], sets[0], sets[1],
                [st, good, keep], compare=[ucur, counts, st, good, keep])


def wide_eig(ctx):
    """rp = 128, n = 65 on three tiles: the matrices of test_wide_eig, mode 0."""
    from tests import tile_stage_ref as R
    from tests.test_gpu_tile_kernels_wide import _eig_mats

    torch, rp, n, n_t = _t(), 128, 65, 3
    sets = [[np.nan_to_num(R.antisymmetric_split(_eig_mats(_rng("weig", s), n, n_t, 5), rp, _rng("anti", s)), nan=0.0)]
            for s in "AB"]
    G = _empty(ctx, sets[0][0].shape, torch.float64)
    Nout, lam = _empty(ctx, (n_t, rp, rp), torch.float64), _empty(ctx, (n_t, rp), torch.float64)

    def run(cx, ws, nb):
        return cx.lib.pmdk_wide_eig(cx.handle, P(G), 2, rp, n, 0, 0.0, P(Nout), P(lam), n_t, ws, nb)

    return Case(ctx, "pmdk_wide_eig_workspace_bytes", (n, n_t), run, [G], sets[0], sets[1], [Nout, lam])


# ---------------------------------------------------------------------------------------------------------------------
# consumers of a decomposition (their own tests hand over an exactly sized buffer, all but one without a guard behind it)
def grid_components(ctx):
    torch, d1, d2 = _t(), 13, 37
    sets = [[_rng("cc", s).integers(0, 16, size=(d1, d2)).astype(np.uint8)] for s in "AB"]
    edges, label = _empty(ctx, (d1, d2), torch.uint8), _empty(ctx, (d1, d2), torch.int32)

    def run(cx, ws, nb):
        return cx.lib.pmd_grid_components(cx.handle, d1, d2, P(edges), P(label), ws, nb)

    return Case(ctx, "pmd_grid_components_workspace_bytes", (d1, d2), run, [edges], sets[0], sets[1], [label])


def oasis_ar1(ctx):
    """Seven problems on five traces of 300 frames, every output requested."""
    torch, Tn, K, n = _t(), 300, 5, 7
    g = np.array([0.95, 0.9, 0.8, 0.97, 0.5, 0.85, 0.99])
    pw_h = _f32(g[:, None] ** np.arange(Tn + 1)[None, :])
    par_h = _f32(np.stack([g, np.full(n, 0.3), np.array([0, 0, 0.2, 0, 0, 0.1, 0]), np.full(n, 0.1)], axis=1).reshape(-1))
    sets = []
    for s in "AB":
        rng = _rng("oasis", s)
        spikes = (rng.random((Tn, K)) < 0.05) * rng.uniform(0.5, 2.0, (Tn, K))
        c = np.zeros((Tn, K))
        for t in range(Tn):
            c[t] = (0.9 * c[t - 1] if t else 0) + spikes[t]
        sets.append([_f32(c + 0.1 + 0.2 * rng.standard_normal((Tn, K)))])
    Y = _empty(ctx, (Tn, K))
    col = torch.from_numpy(np.array([0, 1, 2, 3, 4, 2, 0], dtype=np.int32)).to(ctx.device)
    par, pw = torch.from_numpy(par_h).to(ctx.device), torch.from_numpy(pw_h).to(ctx.device)
    pw_row = torch.arange(n, dtype=torch.int32, device=ctx.device)
    Cc, S = _empty(ctx, (Tn, n)), _empty(ctx, (Tn, n))
    rss, pools = _empty(ctx, (n,), torch.float64), _empty(ctx, (n,), torch.int32)

    def run(cx, ws, nb):
        return cx.lib.pmd_oasis_ar1(cx.handle, P(Y), K, Tn, n, P(col), P(par), P(pw_row), P(pw), Tn + 1, P(Cc), n, P(S), n, P(rss),
                                    P(pools), ws, nb)

    return Case(ctx, "pmd_oasis_ar1_workspace_bytes", (Tn, n), run, [Y], sets[0], sets[1], [Cc, S, rss, pools])


def shift_correlate(ctx):
    n, d1, d2, my, mx = 5, 48, 56, 4, 4
    h, w, ns = d1 - 2 * my, d2 - 2 * mx, (2 * my + 1) * (2 * mx + 1)
    sets = []
    for s in "AB":
        rng = _rng("shift", s)
        tp = rng.standard_normal((h, w))
        sets.append([_f32(rng.standard_normal((n, d1, d2))), _f32(tp - tp.mean())])
    X, tp, surf = _empty(ctx, (n, d1, d2)), _empty(ctx, (h, w)), _empty(ctx, (n * ns,))

    def run(cx, ws, nb):
        return cx.lib.pmd_shift_correlate(cx.handle, P(X), 0, d1 * d2, d2, 0, 0, n, d1, d2, my, mx, P(tp), P(surf), ws, nb)

    return Case(ctx, "pmd_shift_correlate_workspace_bytes", (n, d1, d2, my, mx), run, [X, tp], sets[0], sets[1], [surf])


def patch_correlate(ctx):
    from localmd_amd import piecewise as PW

    torch, n, d1, d2 = _t(), 3, 64, 80
    pg = PW.PatchGrid(d1, d2, (4, 4), (2, 2), (16, 16), (8, 8))
    (my, mx), (ey, ex), (ph, pw) = pg.max_shift, pg.max_deviation, pg.patch
    ns = (2 * ey + 1) * (2 * ex + 1)
    sets = []
    for s in "AB":
        rng = _rng("patch", s)
        tp = rng.standard_normal((pg.P, ph, pw))
        sets.append([_f32(rng.standard_normal((n, d1, d2))), _f32(tp - tp.mean(axis=(1, 2), keepdims=True)),
                     rng.integers(-my, my + 1, size=(n, 2)).astype(np.int32)])
    X, tp, centre = _empty(ctx, (n, d1, d2)), _empty(ctx, (pg.P, ph, pw)), _empty(ctx, (n, 2), torch.int32)
    ys = torch.from_numpy(np.ascontiguousarray(pg.starts[0], dtype=np.int32)).to(ctx.device)
    xs = torch.from_numpy(np.ascontiguousarray(pg.starts[1], dtype=np.int32)).to(ctx.device)
    surf = _empty(ctx, (n * pg.P * ns,))
    geom = (d1, d2, my, mx, ey, ex, ph, pw, pg.gy, pg.gx)

    def run(cx, ws, nb):
        return cx.lib.pmd_patch_correlate(cx.handle, P(X), 0, d1 * d2, d2, n, *geom, P(ys), P(xs), P(centre), P(tp), P(surf), ws, nb)

    return Case(ctx, "pmd_patch_correlate_workspace_bytes", (n, *geom), run, [X, tp, centre], sets[0], sets[1], [surf])


def diag_moments(which):
    """pmd_neighbour_moments or pmd_lag_moments of 1025 frames (two slices of 1024)."""
    def build(ctx):
        torch, Tn, d1, d2, lag = _t(), 1025, 9, 31, 1
        D = d1 * d2
        sets = []
        for s in "AB":
            A = _f32(_rng("diag", s).standard_normal((Tn, D)) + 3.0)
            sets.append([A, A[0].copy()])
        A, ref = _empty(ctx, (Tn, D)), _empty(ctx, (D,))
        mom = _empty(ctx, (10 if which == "neighbour" else 5, D), torch.float64)

        def run(cx, ws, nb):
            if which == "neighbour":
                return cx.lib.pmd_neighbour_moments(cx.handle, P(A), None, P(ref), Tn, d1, d2, 0, P(mom), ws, nb)
            return cx.lib.pmd_lag_moments(cx.handle, P(A), P(ref), Tn, D, lag, 0, P(mom), ws, nb)

        return Case(ctx, "pmd_diag_workspace_bytes", (Tn, D), run, [A, ref], sets[0], sets[1], [mom])

    return build


def diag_fused(ctx):
    """The first call of test_fused_float (frames [0, 512) of 700, fp32, lag 3): the moments are added to, so they are an
    input (zeros) as well as a result."""
    from tests.test_gpu_diag_kernels import _float_case

    torch, Tn, d1, d2, lag, n = _t(), 700, 9, 31, 3, 512
    D = d1 * d2
    y, w, _, mean = _float_case(Tn, d1, d2)
    zeros = np.zeros((35, D))
    sets = [[y.reshape(Tn, D).copy(), w.reshape(Tn, D).copy(), mean.reshape(-1).copy(), zeros],
            [np.ascontiguousarray(y.reshape(Tn, D)[::-1]), np.ascontiguousarray(w.reshape(Tn, D)[::-1] * np.float32(0.5)),
             mean.reshape(-1) + np.float32(1.0), zeros]]
    Y, W, M = _empty(ctx, (Tn, D)), _empty(ctx, (Tn, D)), _empty(ctx, (D,))
    mom, ref, fss = _empty(ctx, (35, D), torch.float64), _empty(ctx, (3, D)), _empty(ctx, (Tn,), torch.float64)

    def run(cx, ws, nb):
        return cx.lib.pmd_diag_fused_accumulate(cx.handle, P(Y), 0, 0, P(W), None, lag, 0, n, Tn, d1, d2, P(M), P(ref), P(mom),
                                                P(fss), ws, nb)

    return Case(ctx, "pmd_diag_fused_workspace_bytes", (n, D), run, [Y, W, M, mom], sets[0], sets[1], [ref, fss],
                compare=[mom, ref, fss])


def group_project(ctx):
    """The kernel case of test_gpu_projection (every (r, p) block of its grid and three dense columns split over the
    partial-sum workspace) on three fp32 frames."""
    from localmd_amd import projection as PJ
    from tests.test_gpu_projection import _kernel_case, _movie

    u, fov = _kernel_case()
    dt = PJ.DeviceTables(ctx, PJ.group_tables(u, fov, "C"))
    assert dt.n_partial_rows > 0
    n, D, ldz = 3, fov[0] * fov[1], 6
    sets = [list(_movie(n, D, np.float32, _rng("gp", s))) for s in "AB"]
    y, mean, std, Z = _empty(ctx, (n, D)), _empty(ctx, (D,)), _empty(ctx, (D,)), _empty(ctx, (dt.n_cols, ldz))

    def run(cx, ws, nb):
        return cx.lib.pmd_group_project(cx.handle, P(y), 0, n, D, P(mean), P(std), dt.n_groups, P(dt.groups), P(dt.pix), P(dt.a),
                                        dt.n_partial_rows, dt.n_wide, P(dt.wide), P(Z), ldz, ws, nb)

    return Case(ctx, "pmd_group_project_workspace_bytes", (dt.n_partial_rows, n), run, [y, mean, std], sets[0], sets[1], [Z])


def roi_gather(ctx):
    """The float-weight ROI set of test_gpu_traces in segments of 128 pixels (split ROIs: a partial-sum workspace) on 65
    fp32 frames."""
    from localmd_amd import traces as TR
    from tests import test_gpu_traces as G

    torch = _t()
    t = TR.roi_tables(G._float_weights(), (G.D1, G.D2), "C", "mean", seg=128)
    assert t["n_partial_rows"] > 0 and len(t["split"]) >= 1
    n, D, K = 65, G.D, t["K"]
    sets = [[_f32(900.0 + 8.0 * _rng("roi", s).standard_normal((n, D)))] for s in "AB"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)
    segs, split, pix, w = dev(t["segs"].reshape(-1)), dev(t["split"].reshape(-1)), dev(t["pix"]), dev(t["w"])
    Y, out = _empty(ctx, (n, D)), _empty(ctx, (K, n))

    def run(cx, ws, nb):
        return cx.lib.pmd_roi_gather(cx.handle, P(Y), 0, n, D, len(t["segs"]), P(segs), P(pix), P(w), t["n_partial_rows"],
                                     len(t["split"]), P(split), P(out), n, ws, nb)

    return Case(ctx, "pmd_roi_gather_workspace_bytes", (t["n_partial_rows"], n), run, [Y], sets[0], sets[1], [out])


CONSUMERS = {"grid_components": grid_components, "oasis_ar1": oasis_ar1, "shift_correlate": shift_correlate,
             "patch_correlate": patch_correlate, "diag_moments-neighbour": diag_moments("neighbour"),
             "diag_moments-lag": diag_moments("lag"), "diag_fused": diag_fused, "group_project": group_project,
             "roi_gather": roi_gather}


# ---------------------------------------------------------------------------------------------------------------------
# workspace-free calls of the stream and context tests
def gemm(m, n, k):
    def build(ctx):
        sets = []
        for s in "AB":
            rng = _rng("gemm", m, n, k, s)
            sets.append([_f32(rng.standard_normal((m, k))), _f32(rng.standard_normal((k, n)) + 0.3)])
        A, B, Cm = _empty(ctx, (m, k)), _empty(ctx, (k, n)), _empty(ctx, (m, n))

        def run(cx, ws, nb):
            return cx.lib.pmd_gemm(cx.handle, 0, 0, m, n, k, 1.0, P(A), k, P(B), n, 0.0, P(Cm), n)

        return Case(ctx, None, (), run, [A, B], sets[0], sets[1], [Cm])

    return build


def syevd(n):
    def build(ctx):
        from tests.test_gpu_global_stage import _indefinite

        torch, lda = _t(), (n + 3) // 4 * 4
        sets = []
        for s in "AB":
            S = np.zeros((n, lda), dtype=np.float32)
            S[:, :n] = _indefinite(_rng("syevd", n, s), n)[0]
            sets.append([S])
        Ad, w, work, info = _empty(ctx, (n, lda)), _empty(ctx, (n,)), _empty(ctx, (n,)), _empty(ctx, (4,), torch.int32)

        def run(cx, ws, nb):
            return cx.lib.pmdk_syevd(cx.handle, n, P(Ad), lda, P(w), P(work), P(info))

        return Case(ctx, None, (), run, [Ad], sets[0], sets[1], [w, info], compare=[Ad, w, info])

    return build


# name -> builder.  MANDATORY: the rows of sections 1 and 2 (exact size, guards, contents; refusals).
MANDATORY = {
    "orthogonalize-identity-130": orthogonalize(130, 130, False),
    "orthogonalize-M-200x130": orthogonalize(200, 130, True),
    "orthogonalize_factored-200x130": orthogonalize_factored(200, 130),
    "gram_mtgm-131x1": gram_mtgm(131, 1),
    "gram_mtgm-217x90": gram_mtgm(217, 90),
    **{f"chol_inverse-{m}-abs{a}": chol_inverse(m, a) for m in (1, 130, 512, 513, 641) for a in (0, 1)},
    "orthogonalize_chol-700x515": orthogonalize_chol(700, 515),
    "projected_svd-50x300x120": projected_svd(50, 300, 120),
    "projected_svd-50x120x300": projected_svd(50, 120, 300),
    "projected_svd-noP-120x300": projected_svd(0, 120, 300, with_p=False),
    "psvd_finish-130-nc0": psvd_finish(130, 0),
    "psvd_finish-130-nc257": psvd_finish(130, 257),
    "projected_svd_factored-900x300x300x700": projected_svd_factored(900, 300, 300, 700),
    "projected_svd_factored-900x300x120x120": projected_svd_factored(900, 300, 120, 120),
    "stats": stats,
    "stats_stream": stats_stream,
    "bg_project": bg_project,
    "background_rsvd": background_rsvd,
    "threshold_sim": threshold_sim,
    "tiles_decompose": tiles_decompose,
    "tiles_residual": tiles_residual,
    "wide_eig": wide_eig,
}

# Rows without a workspace (sections 4 and 5).  The split-K shape is the issue's; 130 x 70 x 300 is a single rocBLAS sgemm on
# a default context and three fp16-piece products under PMD_GEMM_SPLIT_MIN_GFLOP=0, PMD_GEMM_SPLIT_MIN_DIM=1.
EXTRA = {
    "gemm-130x70x300": gemm(130, 70, 300),
    "gemm-splitk-200x333x70001": gemm(200, 333, 70001),
    "syevd-72": syevd(72),
    "syevd-301": syevd(301),
}
ALL = {**MANDATORY, **CONSUMERS, **EXTRA}

# size function -> the existing test that covers it with a guard behind the buffer, or why there is nothing to cover
COVERED_ELSEWHERE = {
    "pmd_sliding_extremum_work_floats": "tests/test_gpu_baseline.py::_extremum (fresh, exact, guard floats behind it)",
    "pmd_sliding_quantile_work_floats": "always 0 (tests/test_gpu_baseline_quantile.py asserts it): no workspace to test",
}

# Upper bound of what a size function reports beyond what its entry point takes (its additive constants and the arrays it
# counts but does not take, read off the formulas in csrc/): half the reported bytes are certainly too few, and the
# half-size refusal is asserted, whenever reported - reported // 2 exceeds it, and always from 1 MiB on.  The dry-run arenas
# of the tile stage, the threshold simulation and the background rSVD add 4096.
SLACK = {
    "pmd_orthogonalize_workspace_bytes": 4096 + 8192 + 4 * 1024,      # + one uncounted vector of m <= 1024 floats
    "pmd_orthogonalize_factored_workspace_bytes": 8192, "pmd_gram_mtgm_workspace_bytes": 4096,
    "pmd_chol_inverse_workspace_bytes": 8192 + 64, "pmd_projected_svd_workspace_bytes": 2 * 8192 + 16 * 1024,
    "pmd_psvd_finish_workspace_bytes": 16384 + 4096, "pmd_stats_workspace_bytes": 1024, "pmd_stats_stream_workspace_bytes": 1024 + 256,
    "pmd_bg_project_workspace_bytes": 8192, "pmd_background_rsvd_workspace_bytes": 4096, "pmd_threshold_sim_workspace_bytes": 4096,
    "pmd_tiles_workspace_bytes": 4096, "pmd_tiles_residual_workspace_bytes": 4096, "pmdk_wide_eig_workspace_bytes": 4096 + 64,
}


def half_is_too_small(case):
    return case.nbytes >= (1 << 20) or (case.size_fn in SLACK and case.nbytes - case.nbytes // 2 > SLACK[case.size_fn])


SIZE_FUNCTION = {
    "orthogonalize": "pmd_orthogonalize_workspace_bytes", "orthogonalize_factored": "pmd_orthogonalize_factored_workspace_bytes",
    "gram_mtgm": "pmd_gram_mtgm_workspace_bytes", "chol_inverse": "pmd_chol_inverse_workspace_bytes",
    "orthogonalize_chol": "pmd_orthogonalize_chol_workspace_bytes", "projected_svd": "pmd_projected_svd_workspace_bytes",
    "psvd_finish": "pmd_psvd_finish_workspace_bytes", "projected_svd_factored": "pmd_projected_svd_factored_workspace_bytes",
    "stats": "pmd_stats_workspace_bytes", "stats_stream": "pmd_stats_stream_workspace_bytes",
    "bg_project": "pmd_bg_project_workspace_bytes", "background_rsvd": "pmd_background_rsvd_workspace_bytes",
    "threshold_sim": "pmd_threshold_sim_workspace_bytes", "tiles_decompose": "pmd_tiles_workspace_bytes",
    "tiles_residual": "pmd_tiles_residual_workspace_bytes", "wide_eig": "pmdk_wide_eig_workspace_bytes",
    "grid_components": "pmd_grid_components_workspace_bytes", "oasis_ar1": "pmd_oasis_ar1_workspace_bytes",
    "shift_correlate": "pmd_shift_correlate_workspace_bytes", "patch_correlate": "pmd_patch_correlate_workspace_bytes",
    "diag_moments": "pmd_diag_workspace_bytes", "diag_fused": "pmd_diag_fused_workspace_bytes",
    "group_project": "pmd_group_project_workspace_bytes", "roi_gather": "pmd_roi_gather_workspace_bytes",
}


def size_function_of(row):
    """The size function of a MANDATORY or CONSUMERS row (rows are named <entry point>[-shape])."""
    return SIZE_FUNCTION[row.split("-")[0]]
