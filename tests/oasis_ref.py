"""
NumPy restatement of the OASIS AR(1) solver (test infrastructure only): ``oasis_ar1`` is the arithmetic stated for
pmd_oasis_ar1 in include/pmd_hip.h, operation by operation.  With ``dtype=np.float32`` every operation is rounded to
fp32 on its own, as on the device, and the result is the kernel's bit for bit (the emulation); with ``np.float64`` it is
the reference the emulation is measured against.  ``nnls_ref`` states the same optimisation problem as a non-negative
least-squares problem for scipy, ``deconvolve_ref`` drives the package's own penalty search with the emulation, and
``planted`` makes the seeded test traces.
"""
import functools
import importlib

import numpy as np

DX = importlib.import_module("localmd_amd.deconvolve")     # the module: the package exports the function under the same name


def power_table(g, T, dtype=np.float32):
    """pw[l] = g^l, l = 0 .. T.  fp32: the table the device reads (the float64 power of the fp32 g rounded once, 0 below
    FLT_MIN).  float64: the plain powers of g."""
    if dtype == np.float32:
        return DX.power_table(g, T)
    return np.float64(g) ** np.arange(int(T) + 1, dtype=np.float64)


def oasis_ar1(y, g, lam, s_min=0.0, b=0.0, dtype=np.float32, pw=None):
    """(c, s, rss, n_pools) of one problem: c, s (T,) ``dtype``, rss float64, n_pools int."""
    single = dtype == np.float32
    f = np.float32 if single else float          # Python floats are IEEE doubles: the float64 form, only faster
    y_arr = np.asarray(y, dtype=dtype)
    T = len(y_arr)
    g, lam, s_min, b = f(g), f(lam), f(s_min), f(b)
    pw_arr = power_table(g, T, dtype) if pw is None else np.asarray(pw, dtype=dtype)
    ys, pws = [f(v) for v in y_arr], [f(v) for v in pw_arr]
    one, zero = f(1.0), f(0.0)
    with np.errstate(all="ignore"):
        mu = lam * (one - g)
        V, W, T0, L = [], [], [], []
        for t in range(T):
            V.append((ys[t] - b) - (mu if t < T - 1 else lam))
            W.append(one), T0.append(t), L.append(1)
            while len(V) >= 2:
                q = pws[L[-2]]
                if not V[-1] < V[-2] * q + s_min:
                    break
                num = W[-2] * V[-2] + (q * W[-1]) * V[-1]
                den = W[-2] + (q * q) * W[-1]
                V[-2], W[-2] = num / den, den
                L[-2] += L[-1]
                V.pop(), W.pop(), T0.pop(), L.pop()
        c, s = np.zeros(T, dtype=dtype), np.zeros(T, dtype=dtype)
        for k in range(len(V)):
            vp = V[k] if V[k] > 0 else zero
            c[T0[k]:T0[k] + L[k]] = dtype(vp) * pw_arr[:L[k]]
            if k >= 1:
                d = c[T0[k]] - dtype(g) * c[T0[k] - 1]
                s[T0[k]] = d if d > 0 else 0
        d = (y_arr - (c + dtype(b))).astype(np.float64)
        rss = float(np.cumsum(d * d)[-1])        # one chain in ascending t
    return c, s, rss, len(V)


def nnls_ref(y, g, lam, b=0.0):
    """(c, s) float64 of the same problem as non-negative least squares: with K the lower-triangular matrix g^(t - tau),
    c = K s and 1/2 |K s + b - y|^2 + lam sum s = 1/2 |K s - y'|^2 + const for y' = y - b - mu (lam at the last
    frame), mu = lam (1 - g); s[0] is the free start c[0] >= 0 here as in the solver, which clips pool values at 0."""
    import scipy.optimize

    y = np.asarray(y, dtype=np.float64)
    T = len(y)
    pen = np.full(T, lam * (1.0 - g))
    pen[-1] = lam
    t = np.arange(T)
    K = np.tril(np.float64(g) ** np.maximum(t[:, None] - t[None, :], 0))
    s, _ = scipy.optimize.nnls(K, y - b - pen, maxiter=30 * T)
    return K @ s, s


def deconvolve_ref(traces, g, noise, lam=None, s_min=0.0, baseline=0.0, rounds=5, points=8, dtype=np.float32):
    """What localmd_amd.deconvolve returns for given ``g`` and ``noise`` ((K,) each), as a dict, with the package's own
    search_lambda driven by ``oasis_ar1`` in ``dtype`` as ``solve``."""
    y = np.ascontiguousarray(traces, dtype=np.float32)
    K, T = y.shape
    g32 = np.broadcast_to(np.asarray(g, dtype=np.float32), (K,))
    sm = np.broadcast_to(np.asarray(s_min, dtype=np.float32), (K,))
    b = np.broadcast_to(np.asarray(baseline, dtype=np.float32), (K,))
    noise = np.broadcast_to(np.asarray(noise, dtype=np.float64), (K,))
    tables = [power_table(g32[k], T, dtype) for k in range(K)]

    def one(k, lm):
        return oasis_ar1(y[k], g32[k], lm, sm[k], b[k], dtype, tables[k])

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
def planted(seed, T=3000, g=0.95, sigma=0.3, rate=0.015):
    """(y (T,) float32, times, amplitudes): an AR(1) trace with events at ``times`` (rate per frame, amplitudes uniform
    in 0.5 .. 1.5, none in the first or last five frames, at least three frames apart) plus white noise sigma."""
    rng = np.random.default_rng(seed)
    times = np.nonzero(rng.random(T) < rate)[0]
    times = times[(times >= 5) & (times < T - 5)]
    times = times[np.concatenate([[True], np.diff(times) >= 3])[:len(times)]]
    amps = rng.uniform(0.5, 1.5, len(times))
    s = np.zeros(T)
    s[times] = amps
    c = np.zeros(T)
    for t in range(T):
        c[t] = (g * c[t - 1] if t else 0.0) + s[t]
    y = (c + sigma * rng.standard_normal(T)).astype(np.float32)
    y.setflags(write=False)
    return y, times, amps


def planted_property(spikes, times, amps, sigma):
    """(hit, big, false_pos): of the ``big`` planted events above 4 sigma, ``hit`` have estimated spikes within +-1 frame
    summing to more than a third of their amplitude; ``false_pos`` estimated spikes above 3 sigma lie farther than one
    frame from every planted event."""
    spikes = np.asarray(spikes, dtype=np.float64)
    T = len(spikes)
    big = [(t, a) for t, a in zip(times, amps) if a > 4 * sigma]
    hit = sum(spikes[max(0, t - 1):t + 2].sum() > a / 3 for t, a in big)
    near = np.zeros(T, dtype=bool)
    for t in times:
        near[max(0, t - 1):t + 2] = True
    return hit, len(big), int(np.sum((spikes > 3 * sigma) & ~near))
