"""
NumPy restatement of the OASIS AR(2) solver (test infrastructure only): ``oasis_ar2`` is the arithmetic stated for
pmd_oasis_ar2 in include/pmd_hip.h, operation by operation.  With ``dtype=np.float32`` every operation is rounded to
fp32 on its own, as on the device, and the result is the kernel's bit for bit (the emulation); with ``np.float64`` it is
the reference the emulation is measured against.  ``nnls_ref2`` states the same optimisation problem as a non-negative
least-squares problem for scipy, ``deconvolve_ref2`` drives the package's own penalty search with the emulation, and
``planted2`` makes the seeded test traces.
"""
import functools
import importlib

import numpy as np

DX = importlib.import_module("localmd_amd.deconvolve")     # the module: the package exports the function under the same name


def tables(g1, g2, T, dtype=np.float32):
    """(3, T + 2): H[i] = h_{i-1}, HH[l], HK[l].  fp32: the tables the device reads (DX.ar2_tables).  float64: the plain
    recursion and sums, unrounded and with nothing set to 0."""
    if dtype == np.float32:
        return DX.ar2_tables(g1, g2, T)
    g1, g2, T = float(g1), float(g2), int(T)
    h = np.zeros(T + 2)
    h[1] = 1.0
    for i in range(2, T + 2):
        h[i] = g1 * h[i - 1] + g2 * h[i - 2]
    tab = np.zeros((3, T + 2))
    tab[0] = h
    tab[1, 1:T + 1] = np.cumsum(h[1:T + 1] ** 2)
    tab[2, 1:T + 1] = np.cumsum(h[1:T + 1] * h[:T])
    return tab


def oasis_ar2(y, g1, g2, lam, s_min=0.0, b=0.0, dtype=np.float32, tab=None, pools=False):
    """(c, s, rss, n_pools) of one problem: c, s (T,) ``dtype``, rss float64, n_pools int.  With ``pools`` a fifth entry:
    the final pools as a list of (t0, l, v, gw)."""
    single = dtype == np.float32
    f = np.float32 if single else float          # Python floats are IEEE doubles: the float64 form, only faster
    y_arr = np.asarray(y, dtype=dtype)
    T = len(y_arr)
    g1, g2, lam, s_min, b = f(g1), f(g2), f(lam), f(s_min), f(b)
    tab_arr = tables(g1, g2, T, dtype) if tab is None else np.asarray(tab, dtype=dtype)
    ys = [f(v) for v in y_arr]
    H, HH, HK = ([f(v) for v in row] for row in tab_arr[:3])
    zero = f(0.0)
    with np.errstate(all="ignore"):
        one_g1 = f(1.0) - g1
        mu = lam * (one_g1 - g2)
        mu1 = lam * one_g1
        V, W, N, M, T0, L = [], [], [], [], [], []

        def gw_of(k):                            # g2 * w of the pool under pool k
            return g2 * (W[k - 1] if k >= 1 else zero)

        for t in range(T):
            x = (ys[t] - b) - (mu if t < T - 2 else (mu1 if t == T - 2 else lam))
            xv = x if V or x > 0 else zero       # the bottom pool's value is clipped, its sum N is not
            V.append(xv), W.append(xv), N.append(x), M.append(zero), T0.append(t), L.append(1)
            while len(V) >= 2:
                k = len(V) - 2
                m, gw = L[k], gw_of(k)
                pred = H[m + 1] * V[k] + H[m] * gw
                if not V[-1] < pred + s_min:
                    break
                gm = g2 * M[-1]
                an = H[m + 1] * N[-1] + H[m] * gm
                bm = H[m] * N[-1] + H[m - 1] * gm
                N[k], M[k] = N[k] + an, M[k] + bm
                L[k] += L[-1]
                V.pop(), W.pop(), N.pop(), M.pop(), T0.pop(), L.pop()
                ln = L[k]
                v = (N[k] - gw * HK[ln]) / HH[ln]
                if k == 0:
                    v = v if v > 0 else zero
                V[k] = v
                W[k] = H[ln] * v + H[ln - 1] * gw
        c, s = np.zeros(T, dtype=dtype), np.zeros(T, dtype=dtype)
        final = []
        Ha = np.asarray(H, dtype=dtype)
        for k in range(len(V)):
            gw = gw_of(k)
            ln = L[k]
            final.append((T0[k], ln, V[k], gw))
            c[T0[k]:T0[k] + ln] = Ha[1:ln + 1] * dtype(V[k]) + Ha[:ln] * dtype(gw)
            if k >= 1:
                t = T0[k]
                d = c[t] - dtype(g1) * c[t - 1]
                if t >= 2:
                    d = d - dtype(g2) * c[t - 2]
                s[t] = d if d > 0 else 0
        d = (y_arr - (c + dtype(b))).astype(np.float64)
        rss = float(np.cumsum(d * d)[-1])        # one chain in ascending t
    out = (c, s, rss, len(V))
    return out + (final,) if pools else out


def objective(y, c, g1, g2, lam, b=0.0):
    """1/2 |c + b - y|^2 + lam sum_t s_t in float64 with s_t = c_t - g1 c_{t-1} - g2 c_{t-2} (s_0 = c_0), and min s."""
    y, c = np.asarray(y, dtype=np.float64), np.asarray(c, dtype=np.float64)
    s = c.copy()
    s[1:] -= g1 * c[:-1]
    s[2:] -= g2 * c[:-2]
    r = c + b - y
    return 0.5 * float(r @ r) + lam * float(s.sum()), float(s.min())


def nnls_ref2(y, g1, g2, lam, b=0.0):
    """(c, s) float64 of the same problem as non-negative least squares: with K the lower-triangular Toeplitz matrix
    h_{t - tau}, c = K s and 1/2 |K s + b - y|^2 + lam sum s = 1/2 |K s - y'|^2 + const for y' = y - b - K^-T lam 1,
    that is the penalties mu_t of the solver; s[0] is the free start c[0] >= 0."""
    import scipy.linalg
    import scipy.optimize

    y = np.asarray(y, dtype=np.float64)
    T = len(y)
    pen = np.full(T, lam * (1.0 - g1 - g2))
    if T >= 2:
        pen[-2] = lam * (1.0 - g1)
    pen[-1] = lam
    h = tables(g1, g2, T, np.float64)[0][1:T + 1]
    K = scipy.linalg.toeplitz(h, np.zeros(T))
    s, _ = scipy.optimize.nnls(K, y - b - pen, maxiter=30 * T)
    return K @ s, s


def deconvolve_ref2(traces, g, noise, lam=None, s_min=0.0, baseline=0.0, rounds=5, points=8, dtype=np.float32):
    """What localmd_amd.deconvolve(p=2) returns for given ``g`` ((K, 2) or a pair) and ``noise`` ((K,)), as a dict, with
    the package's own search_lambda driven by ``oasis_ar2`` in ``dtype`` as ``solve``."""
    y = np.ascontiguousarray(traces, dtype=np.float32)
    K, T = y.shape
    g32 = np.broadcast_to(np.asarray(g, dtype=np.float32), (K, 2))
    sm = np.broadcast_to(np.asarray(s_min, dtype=np.float32), (K,))
    b = np.broadcast_to(np.asarray(baseline, dtype=np.float32), (K,))
    noise = np.broadcast_to(np.asarray(noise, dtype=np.float64), (K,))
    tabs = [tables(g32[k, 0], g32[k, 1], T, dtype) for k in range(K)]

    def one(k, lm):
        return oasis_ar2(y[k], g32[k, 0], g32[k, 1], lm, sm[k], b[k], dtype, tabs[k])

    def solve(idx, lams):
        return np.array([one(int(k), lm)[2] for k, lm in zip(idx, lams)], dtype=np.float64)

    if lam is None:
        lam32, evaluations = DX.search_lambda(solve, noise ** 2 * T, DX.lambda_ceiling(y, g32, b), rounds, points)
    else:
        lam32 = np.broadcast_to(np.asarray(lam, dtype=np.float32), (K,)).copy()
        evaluations = np.zeros(K, dtype=np.int64)
    out = [one(k, lam32[k]) for k in range(K)]
    return {"calcium": np.stack([o[0] for o in out]), "spikes": np.stack([o[1] for o in out]), "lam": lam32,
            "rss": np.array([o[2] for o in out]), "n_pools": np.array([o[3] for o in out], dtype=np.int32),
            "evaluations": evaluations + 1, "target": noise ** 2 * T}


@functools.lru_cache(maxsize=None)
def planted2(seed, T=3000, d=0.95, r=0.5, sigma=0.3, rate=0.015):
    """(y (T,) float32, times, amplitudes): an AR(2) trace with roots d >= r and events at ``times`` (rate per frame,
    amplitudes uniform in 0.5 .. 1.5, none in the first or last five frames, at least three frames apart) plus white
    noise sigma.  The response is scaled to unit peak per unit spike, so ``amplitudes`` are peak heights; the spikes of
    the model are ``amplitudes / max_j h_j``."""
    rng = np.random.default_rng(seed)
    times = np.nonzero(rng.random(T) < rate)[0]
    times = times[(times >= 5) & (times < T - 5)]
    times = times[np.concatenate([[True], np.diff(times) >= 3])[:len(times)]]
    amps = rng.uniform(0.5, 1.5, len(times))
    g1, g2 = d + r, -d * r
    s = np.zeros(T)
    s[times] = amps
    c = np.zeros(T)
    for t in range(T):
        c[t] = (g1 * c[t - 1] if t else 0.0) + (g2 * c[t - 2] if t > 1 else 0.0) + s[t]
    c /= tables(g1, g2, 200, np.float64)[0].max()
    y = (c + sigma * rng.standard_normal(T)).astype(np.float32)
    y.setflags(write=False)
    return y, times, amps
