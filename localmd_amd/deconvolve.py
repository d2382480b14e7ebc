"""
Spike inference: the activity behind each ROI trace, by OASIS for an AR(1) model (Friedrich, Zhou & Paninski 2017,
Alg. 1) or, with ``p=2``, for an AR(2) model with a finite rise time (Alg. 3).

``deconvolve(traces)`` takes (K, T) time courses (those of demix, extract_traces or trace_baseline) and returns, per
trace, the denoised calcium ``c``, the non-negative spike train ``s_t = c_t - g c_{t-1}`` and the decay ``g``, noise
level ``sigma`` and penalty ``lam`` it used.  For one trace it minimises ``1/2 |c + b - y|^2 + lam sum_t s_t`` over
``s >= 0`` (``s_min > 0``: the hard-threshold variant of the paper).  With ``p=2`` the spikes are
``s_t = c_t - g1 c_{t-1} - g2 c_{t-2}`` for a pair ``g = (g1, g2) = (d + r, -d r)`` with real roots ``0 <= r <= d < 1``
(decay and rise); the pooled solver is greedy: close to the optimum, and the optimum itself when ``g2 = 0``.

The solve is sequential along time but independent across traces and across candidate penalties, so the device runs one
lane per (trace, penalty) problem (``pmd_oasis_ar1``, csrc/oasis.hip, and ``pmd_oasis_ar2``, csrc/oasis2.hip; the
arithmetic is stated in include/pmd_hip.h and restated in tests/oasis_ref.py and tests/oasis2_ref.py, which reproduce it
bit for bit).  Every scalar decision is float64 host code around it:

* ``noise=None``: the Welch upper-half-band sigma a pixel gets (``pmd_stats`` on the (T, K) matrix, 1024-frame chunks).
* ``g=None``: ``estimate_decay`` (``estimate_ar2`` for p = 2), from the first autocovariances with the noise taken off
  lag 0.
* ``lam=None``: the largest penalty whose residual stays within the noise, ``rss(lam) <= sigma^2 T``, by an m-section
  search (``search_lambda``).  Every round is one batch of (trace, candidate) problems over all traces still searching.

The powers of g come from a host table (``power_table``), one row per trace, shared by all its candidates; for p = 2
three rows per trace (``ar2_tables``): the impulse response and the running sums of its squares and lagged products.

Device memory (``deconvolve_device_bytes``): the traces, the two outputs and the tables stay resident, ``12 K T +
4 K (T + 1)`` bytes (``12 K T + 12 K (T + 2)`` for p = 2); the solver's pool stacks are ``12 T`` (``24 T``) bytes per
problem in flight and are capped at ``max_workspace_bytes``: a round is split into launches that fit (``launch_plan``),
and no bit depends on the split.

Everything that differs between the two orders (entry point, pool and table layout, the ``par`` columns, the check and
the estimate of g, the penalty ceiling) is one ``_Order`` record each in ``_ORDERS``; a further model is a further record
there and nothing else in this module.

Out of scope: joint optimisation of g or of the baseline, complex roots, and an exact AR(2) solve.
"""
from typing import Callable, NamedTuple

import numpy as np

from . import _stream
from ._movie import _device_free_bytes
from ._stream import _check_count, device_context

LAGS = 5                    # autocovariance lags estimate_decay fits
LAGS2 = 10                  # autocovariance lags estimate_ar2 fits
MIN_NOISE_FRAMES = 256      # the Welch window: pmd_stats makes no estimate below it
G_MAX = 0.9999              # the ceiling of an estimated decay
FLT_MIN = float(np.finfo(np.float32).tiny)


class Deconvolved:
    """Result of deconvolve: ``calcium`` and ``spikes`` ((K, T) float32), and per trace ``g``, ``noise``, ``lam``,
    ``baseline`` (float32 as the solver read them; ``noise`` float64; ``g`` is (K,) for p = 1 and (K, 2), the pairs
    (g1, g2), for p = 2), ``rss`` (float64, |y - c - b|^2), ``n_pools`` and ``evaluations`` (the number of solves the
    trace took)."""

    def __init__(self, calcium, spikes, g, noise, lam, baseline, rss, n_pools, evaluations):
        self.calcium, self.spikes = calcium, spikes
        self.g, self.noise, self.lam, self.baseline = g, noise, lam, baseline
        self.rss, self.n_pools, self.evaluations = rss, n_pools, evaluations

    def __repr__(self):
        return "Deconvolved({} traces, {} frames)".format(*self.calcium.shape)


# ---- host side: tables, estimates, the search, the plan (no device work) ---------------------------------------------
def power_table(g, T):
    """pw[l] = g^l for l = 0 .. T as the solver reads it: the float64 power of the fp32 value of g, rounded once to
    fp32, and exactly 0 below the smallest normal fp32 number.  ``g`` a scalar ((T + 1,)) or (K,) ((K, T + 1))."""
    g64 = np.asarray(g, dtype=np.float32).astype(np.float64)
    p = g64[..., None] ** np.arange(int(T) + 1, dtype=np.float64)
    return np.where(p < FLT_MIN, 0.0, p).astype(np.float32)


def estimate_decay(traces, noise, lags=LAGS):
    """The AR(1) decay of every row of ``traces`` ((K, T)) given its noise level, float64: with the autocovariances
    ``xc[0 .. lags]`` of the mean-removed trace (divided by T) and ``a_tau = xc[tau - 1] - noise^2 [tau = 1]``, the
    least-squares g of ``xc[tau] = g a_tau``, ``sum a_tau xc[tau] / sum a_tau^2``, clipped to [0, 0.9999]."""
    x = np.atleast_2d(np.asarray(traces, dtype=np.float64))
    K, T = x.shape
    lags = int(lags)
    if lags < 1 or T <= lags:
        raise ValueError("estimate_decay needs 1 <= lags < T, got lags {} on {} frames".format(lags, T))
    s2 = np.broadcast_to(np.asarray(noise, dtype=np.float64), (K,)) ** 2
    x = x - x.mean(axis=1, keepdims=True)
    xc = np.stack([np.einsum("kt,kt->k", x[:, :T - l], x[:, l:]) / T for l in range(lags + 1)], axis=1)
    a = xc[:, :lags].copy()
    a[:, 0] -= s2
    den = np.einsum("kl,kl->k", a, a)
    num = np.einsum("kl,kl->k", a, xc[:, 1:])
    g = np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)
    return np.clip(g, 0.0, G_MAX)


def ar2_violation(g1, g2):
    """The condition of the admissible set of the AR(2) solver that the pair(s) ``g1, g2`` miss, or None: the roots
    ``d >= r`` of ``z^2 - g1 z - g2`` are real with ``0 <= r <= d < 1``.  Evaluated in float64 on the fp32 values."""
    g1 = np.asarray(g1, dtype=np.float32).astype(np.float64)
    g2 = np.asarray(g2, dtype=np.float32).astype(np.float64)
    for ok, rule in ((np.isfinite(g1) & np.isfinite(g2), "finite g1, g2"),
                     (g1 >= 0, "g1 >= 0 (no negative root)"), (g2 <= 0, "g2 <= 0 (no negative root)"),
                     (g1 * g1 + 4.0 * g2 >= 0, "g1^2 + 4 g2 >= 0 (real roots)"),
                     (g1 < 2, "g1 < 2 (roots below 1)"), (1.0 - g1 - g2 > 0, "1 - g1 - g2 > 0 (roots below 1)")):
        if not np.all(ok):
            return rule
    return None


def ar2_from_roots(d, r):
    """(g1, g2) = (d + r, -d r) of the AR(2) model whose impulse response decays with the root ``d`` and rises with the
    root ``r``, ``0 <= r <= d < 1`` (scalars, or arrays of one shape: then a (..., 2) array).  The pair is returned as
    float64 numbers that fp32 holds exactly and that are admissible as fp32: where rounding a double or nearly double
    root, or a pair of roots next to 1, leaves the admissible set, ``r`` is lowered in steps of 2^-12 until it does
    not."""
    d64, r64 = np.broadcast_arrays(np.asarray(d, dtype=np.float64), np.asarray(r, dtype=np.float64))
    if not np.all((r64 >= 0) & (r64 <= d64) & (d64 < 1)):
        raise ValueError("the roots must satisfy 0 <= r <= d < 1, got d = {!r}, r = {!r}".format(d, r))
    if np.any(d64.astype(np.float32) >= 1):
        raise ValueError("d must be below 1 in float32")
    d64, r64 = d64.copy(), r64.copy()
    pair = lambda: np.stack([(d64 + r64).astype(np.float32), (-d64 * r64).astype(np.float32)], axis=-1)   # noqa: E731
    g = pair()
    for _ in range(4096):
        g1, g2 = g[..., 0].astype(np.float64), g[..., 1].astype(np.float64)
        bad = (g1 * g1 + 4.0 * g2 < 0) | (1.0 - g1 - g2 <= 0)
        if not np.any(bad):
            break
        r64 = np.where(bad, np.maximum(0.0, r64 - 2.0 ** -12), r64)
        g = pair()
    return g.astype(np.float64)


def ar2_from_time_constants(tau_rise, tau_decay, frame_rate):
    """ar2_from_roots for an indicator that rises with the time constant ``tau_rise`` and decays with ``tau_decay``
    (seconds, 0 < tau_rise <= tau_decay) sampled at ``frame_rate`` (Hz): d = exp(-1 / (tau_decay rate)),
    r = exp(-1 / (tau_rise rate))."""
    rise, decay, rate = (np.asarray(v, dtype=np.float64) for v in (tau_rise, tau_decay, frame_rate))
    if not np.all((rise > 0) & (decay >= rise) & (rate > 0) & np.isfinite(decay) & np.isfinite(rate)):
        raise ValueError("time constants must satisfy 0 < tau_rise <= tau_decay, and frame_rate > 0")
    return ar2_from_roots(np.exp(-1.0 / (decay * rate)), np.exp(-1.0 / (rise * rate)))


def ar2_tables(g1, g2, T):
    """The three table rows the AR(2) solver reads, (3, T + 2) float32 for scalars and (K, 3, T + 2) for (K,) arrays:
    row 0 ``H[i] = h_{i-1}``, i = 0 .. T + 1, the impulse response ``h_{-1} = 0, h_0 = 1, h_j = g1 h_{j-1} + g2 h_{j-2}``;
    row 1 ``HH[l] = sum_{j<l} h_j^2`` and row 2 ``HK[l] = sum_{j<l} h_j h_{j-1}``, l = 0 .. T (entry T + 1 is 0).  The
    recursion and the sums run in float64 on the fp32 values of g1 and g2; every entry is rounded once to fp32, and
    entries of H below the smallest normal fp32 number are exactly 0."""
    a1 = np.asarray(g1, dtype=np.float32).astype(np.float64)
    a2 = np.asarray(g2, dtype=np.float32).astype(np.float64)
    scalar = a1.ndim == 0 and a2.ndim == 0
    a1, a2 = np.broadcast_arrays(np.atleast_1d(a1), np.atleast_1d(a2))
    T = int(T)
    h = np.zeros((len(a1), T + 2))
    h[:, 1] = 1.0
    for i in range(2, T + 2):
        h[:, i] = a1 * h[:, i - 1] + a2 * h[:, i - 2]
    tab = np.zeros((len(a1), 3, T + 2))
    tab[:, 0] = np.where(h < FLT_MIN, 0.0, h)
    tab[:, 1, 1:T + 1] = np.cumsum(h[:, 1:T + 1] ** 2, axis=1)
    tab[:, 2, 1:T + 1] = np.cumsum(h[:, 1:T + 1] * h[:, :T], axis=1)
    tab = tab.astype(np.float32)
    return tab[0] if scalar else tab


def estimate_ar2(traces, noise, lags=LAGS2):
    """The AR(2) pair of every row of ``traces`` ((K, T)) given its noise level, (K, 2) float64: with the autocovariances
    ``xc[0 .. lags]`` of the mean-removed trace (divided by T), ``a_0 = xc[0] - noise^2`` and ``a_j = xc[j]``, the
    least-squares (g1, g2) of ``xc[tau] = g1 a_{tau-1} + g2 a_{|tau-2|}``, tau = 1 .. lags.  The roots of
    ``z^2 - g1 z - g2`` (a complex pair: its real part twice) are clipped to [0, 0.9999] and ordered d >= r; the result
    is ``ar2_from_roots(d, r)``.  Needs T > lags + 1 and lags >= 2.  The decay is found well, the rise only roughly:
    on planted traces of 10^4 frames at noise 0.3 and unit peaks, d came out within 0.014 and r within 0.15 to 0.33 of
    the truth (roots (0.9, 0.3) to (0.97, 0.8)); pass ``g=`` from the indicator's time constants when they are known."""
    x = np.atleast_2d(np.asarray(traces, dtype=np.float64))
    K, T = x.shape
    lags = int(lags)
    if lags < 2 or T <= lags + 1:
        raise ValueError("estimate_ar2 needs 2 <= lags < T - 1, got lags {} on {} frames".format(lags, T))
    s2 = np.broadcast_to(np.asarray(noise, dtype=np.float64), (K,)) ** 2
    x = x - x.mean(axis=1, keepdims=True)
    xc = np.stack([np.einsum("kt,kt->k", x[:, :T - l], x[:, l:]) / T for l in range(lags + 1)], axis=1)
    a = xc.copy()
    a[:, 0] -= s2
    tau = np.arange(1, lags + 1)
    A = np.stack([a[:, tau - 1], a[:, np.abs(tau - 2)]], axis=2)          # (K, lags, 2)
    g = np.zeros((K, 2))
    for k in range(K):
        if np.all(np.isfinite(A[k])) and np.all(np.isfinite(xc[k])):
            g[k] = np.linalg.lstsq(A[k], xc[k, 1:], rcond=None)[0]
    disc = g[:, 0] ** 2 + 4.0 * g[:, 1]
    root = np.sqrt(np.maximum(disc, 0.0))
    d = np.clip((g[:, 0] + root) / 2.0, 0.0, G_MAX)
    r = np.clip((g[:, 0] - root) / 2.0, 0.0, G_MAX)
    return ar2_from_roots(np.maximum(d, r), np.minimum(d, r))


def lambda_ceiling(y, g, b):
    """The penalty from which on the solution is c = 0, per row of ``y`` ((K, T) float32; g, b (K,) float32):
    ``max(0, max_{t < T - 1} (y_t - b) / (1 - g), y_{T - 1} - b)`` in float64, rounded to fp32.  With ``g`` (K, 2), the
    AR(2) pairs: ``max(0, max_{t < T - 2} (y_t - b) / (1 - g1 - g2), (y_{T - 2} - b) / (1 - g1), y_{T - 1} - b)``.  From
    there on every penalised sample is <= 0.  Where ``1 - g1 <= 0`` the penalty of frame T - 2 is not positive and no
    lam makes that sample <= 0; its term is then ``(y_{T - 2} - b) + g1 (y_{T - 1} - b)``, from which on the last two
    frames pool to a value <= 0 (the last sample alone is <= 0 already, so it merges)."""
    d = np.asarray(y, dtype=np.float64) - np.asarray(b, dtype=np.float64)[:, None]
    g = np.asarray(g, dtype=np.float64)
    hi = np.maximum(0.0, d[:, -1])
    return _ORDERS[2 if g.ndim == 2 else 1].ceiling(d, g, hi).astype(np.float32)


def _ceiling_ar1(d, g, hi):
    if d.shape[1] > 1:
        hi = np.maximum(hi, d[:, :-1].max(axis=1) / (1.0 - g))
    return hi


def _ceiling_ar2(d, g, hi):
    if d.shape[1] > 1:
        w = 1.0 - g[:, 0]
        hi = np.maximum(hi, np.where(w > 0, d[:, -2] / np.where(w > 0, w, 1.0), d[:, -2] + g[:, 0] * d[:, -1]))
    if d.shape[1] > 2:
        hi = np.maximum(hi, d[:, :-2].max(axis=1) / (1.0 - g[:, 0] - g[:, 1]))
    return hi


def _collapsed(lo, hi):
    """No fp32 number lies strictly between lo and hi."""
    return np.nextafter(lo.astype(np.float32), np.float32(np.inf)) >= hi.astype(np.float32)


def search_lambda(solve, target, lam_hi, rounds=5, points=8):
    """The noise-constrained penalty of every trace: the largest lam found with ``rss(lam) <= target``.

    ``solve(idx, lam) -> rss`` solves the problems (trace idx[i], penalty lam[i]) (int64 and float32 arrays of one
    length) and returns their residual sums of squares (float64); it is the only access to the traces, so the same
    function runs on the device and on the emulation.  ``target`` ((K,) float64) is sigma^2 T, ``lam_hi`` ((K,) float32)
    lambda_ceiling.  Round 0 solves lam = 0 and lam = lam_hi for every trace: ``rss(0) >= target`` ends at 0 (the
    trace is already smoother than its noise allows), ``rss(lam_hi) <= target`` ends at lam_hi (the trace is noise).
    Every further round solves the ``points`` candidates ``fl32(lo + (hi - lo) j / (points + 1))`` of every trace
    still searching; on the grid [lo, candidates, hi] the largest entry with rss <= target (lo always qualifies)
    becomes lo and its successor hi.  A trace whose bracket holds no fp32 number any more drops out.
    Returns (lam (K,) float32, evaluations (K,) int64: the solves each trace took)."""
    target = np.asarray(target, dtype=np.float64)
    K, m = len(target), int(points)
    every = np.arange(K, dtype=np.int64)
    lo, hi = np.zeros(K, dtype=np.float32), np.asarray(lam_hi, dtype=np.float32).copy()
    r = np.asarray(solve(np.concatenate([every, every]), np.concatenate([lo, hi])), dtype=np.float64)
    evaluations = np.full(K, 2, dtype=np.int64)
    at_zero = r[:K] >= target
    at_ceiling = ~at_zero & (r[K:] <= target)
    lo[at_ceiling] = hi[at_ceiling]
    active = ~at_zero & ~at_ceiling & ~_collapsed(lo, hi)
    j = np.arange(1, m + 1, dtype=np.float64)
    for _ in range(int(rounds)):
        idx = np.nonzero(active)[0]
        if len(idx) == 0:
            break
        lo64, hi64 = lo[idx].astype(np.float64), hi[idx].astype(np.float64)
        cand = (lo64[:, None] + (hi64 - lo64)[:, None] * j / (m + 1)).astype(np.float32)
        r = np.asarray(solve(np.repeat(idx, m), cand.reshape(-1)), dtype=np.float64).reshape(len(idx), m)
        evaluations[idx] += m
        grid = np.concatenate([lo[idx, None], cand, hi[idx, None]], axis=1)
        ok = r <= target[idx, None]
        best = np.where(ok.any(axis=1), m - np.argmax(ok[:, ::-1], axis=1), 0)     # index on the grid; 0 is lo
        rows = np.arange(len(idx))
        lo[idx], hi[idx] = grid[rows, best], grid[rows, best + 1]
        active[idx] = ~_collapsed(lo[idx], hi[idx])
    return lo, evaluations


def _check_order(p):
    """The _Order record of ``p``."""
    if isinstance(p, (bool, np.bool_)) or p not in (1, 2):
        raise ValueError("p must be 1 (AR(1)) or 2 (AR(2)), got {!r}".format(p))
    return _ORDERS[int(p)]


def workspace_bytes(T, n_prob, p=1):
    """pmd_oasis_ar1_workspace_bytes: the pool stacks of n_prob problems (p = 2: of pmd_oasis_ar2, 24 bytes a pool)."""
    return _check_order(p).pool_bytes * int(T) * int(n_prob)


def launch_plan(n_prob, T, max_workspace_bytes, p=1):
    """[(p0, p1), ...]: the ranges of problems one launch takes each: as many as have their pool stacks within
    ``max_workspace_bytes``, in whole waves of 64 when more than one wave fits.  ValueError when not one problem fits."""
    n_prob, T = int(n_prob), int(T)
    per = int(max_workspace_bytes) // workspace_bytes(T, 1, p)
    if per < 1:
        raise ValueError("max_workspace_bytes = {} does not hold the pool stack of one problem on {} frames: {} bytes "
                         "are the least".format(int(max_workspace_bytes), T, workspace_bytes(T, 1, p)))
    if per > 64:
        per = per // 64 * 64
    return [(p0, min(n_prob, p0 + per)) for p0 in range(0, n_prob, per)]


def deconvolve_device_bytes(*, K, T, problems, max_workspace_bytes, stats_bytes=0, p=1):
    """Device bytes deconvolve holds for K traces of T frames when its largest round has ``problems`` problems.  The
    traces, the calcium, the spikes (12 K T) and the power tables (4 K (T + 1); p = 2: the three table rows,
    12 K (T + 2)) stay resident; the pool stacks of the largest launch of launch_plan and 36 (p = 2: 40) bytes of
    tables per problem of it come on top, and ``stats_bytes``, the workspace of pmd_stats with its two outputs, when the
    noise is estimated."""
    K, T, order = int(K), int(T), _check_order(p)
    largest = max(p1 - p0 for p0, p1 in launch_plan(problems, T, max_workspace_bytes, p))
    need = 12 * K * T + 4 * order.rows * K * order.ldtab(T)
    need += workspace_bytes(T, largest, p) + order.small_bytes * largest
    return need + int(stats_bytes) + (1 << 20)     # the allocator's rounding of the small arrays


def check_fit(need, free):
    _stream.check_fit("deconvolve", need, free, hint=": lower max_workspace_bytes, or pass fewer traces at a time")


def _per_trace(value, K, name, ok, rule):
    """``value`` (a scalar or (K,)) as a (K,) float64 array whose entries all satisfy ``ok``."""
    try:
        a = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("{} must be a number or an array of {} numbers, got {!r}".format(name, K, value)) from None
    if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != K):
        raise ValueError("{} must be a scalar or of shape ({},), got shape {}".format(name, K, a.shape))
    a = np.broadcast_to(a, (K,)).copy()
    if not np.all(ok(a)):
        raise ValueError("{} must satisfy {}".format(name, rule))
    return a


def _check_decay(g, K):
    """``g`` of deconvolve(p=1), a scalar or (K,), as a (K,) float64 array of decays below 1 in float32."""
    g = _per_trace(g, K, "g", lambda v: (v >= 0) & (v < 1), "0 <= g < 1")
    if np.any(g.astype(np.float32) >= 1):
        raise ValueError("g must be below 1 in float32")
    return g


def _check_pairs(g, K):
    """``g`` of deconvolve(p=2), a pair or (K, 2), as a (K, 2) float64 array of admissible pairs."""
    try:
        a = np.asarray(g, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("g must be a pair (g1, g2) or an array of shape ({}, 2) for p = 2, got {!r}".format(K, g)) from None
    if a.shape not in ((2,), (K, 2)):
        raise ValueError("g must be a pair (g1, g2) or of shape ({}, 2) for p = 2, got shape {}".format(K, a.shape))
    a = np.broadcast_to(a, (K, 2)).copy()
    with np.errstate(over="ignore"):
        rule = ar2_violation(a[:, 0], a[:, 1])
    if rule is not None:
        raise ValueError("g = (g1, g2) must satisfy {} in float32: the roots of z^2 - g1 z - g2 are real and lie in "
                         "[0, 1) (ar2_from_roots makes such a pair)".format(rule))
    return a


class _Order(NamedTuple):
    """What an AR order is to this module.  ``g`` is (K,) for p = 1 and (K, 2), the pairs (g1, g2), for p = 2."""
    entry: str              # the C entry point
    pool_bytes: int         # one pool on a problem's stack: (v, w, t0); p = 2: (v, w, N, M, t0) and a spare word
    small_bytes: int        # per problem of a launch: col, par, rss, n_pools (p = 2: and tab_row)
    rows: int               # table rows per trace
    row_extra: int          # a table row has T + row_extra entries
    tables: Callable        # (g fp32, T) -> the (rows K, T + row_extra) fp32 table
    par: Callable           # (g[idx], lam, s_min[idx], b[idx]) -> the columns of the entry point's par, in its order
    check_g: Callable       # (g as given, K) -> g float64, or ValueError
    estimate: Callable      # (traces, noise) -> g float64
    estimate_frames: int    # ... which needs T above this
    ceiling: Callable       # the order's part of lambda_ceiling

    def ldtab(self, T):
        return T + self.row_extra


_ORDERS = {
    1: _Order(entry="pmd_oasis_ar1", pool_bytes=12, small_bytes=36, rows=1, row_extra=1, tables=power_table,
              par=lambda g, lam, s_min, b: (g, lam, s_min, b),
              check_g=_check_decay, estimate=estimate_decay, estimate_frames=LAGS, ceiling=_ceiling_ar1),
    2: _Order(entry="pmd_oasis_ar2", pool_bytes=24, small_bytes=40, rows=3, row_extra=2,
              tables=lambda g, T: ar2_tables(g[:, 0], g[:, 1], T).reshape(-1, T + 2),
              par=lambda g, lam, s_min, b: (g[:, 0], g[:, 1], lam, s_min, b),
              check_g=_check_pairs, estimate=estimate_ar2, estimate_frames=LAGS2 + 1, ceiling=_ceiling_ar2),
}


def check_arguments(traces, g, noise, lam, s_min, baseline, search_rounds, search_points, max_workspace_bytes, p=1):
    """The checked arguments of deconvolve, before any device work: (y (K, T) float32, g, noise, lam (each (K,) float64
    or None; g (K, 2) for p = 2), s_min, baseline ((K,) float32), rounds, points, max_workspace_bytes)."""
    order = _check_order(p)
    a = np.asarray(traces)
    if a.ndim != 2 or a.dtype.kind not in "iuf" or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("traces must be a (K, T) array of numbers with K >= 1 and T >= 1")
    with np.errstate(over="ignore"):
        y = np.ascontiguousarray(a, dtype=np.float32)
    if not np.all(np.isfinite(y)):
        raise ValueError("traces hold values that are not finite in float32")
    K, T = y.shape
    if T >= 2 ** 31 - 1:
        raise ValueError("{} frames are too many: the solver counts frames in 32 bits".format(T))
    finite = np.isfinite
    if g is not None:
        g = order.check_g(g, K)
    if noise is not None:
        noise = _per_trace(noise, K, "noise", lambda v: (v > 0) & finite(v), "noise > 0")
    if lam is not None:
        lam = _per_trace(lam, K, "lam", lambda v: (v >= 0) & finite(v.astype(np.float32)), "lam >= 0")
    s_min = _per_trace(s_min, K, "s_min", lambda v: (v >= 0) & finite(v.astype(np.float32)), "s_min >= 0")
    baseline = _per_trace(baseline, K, "baseline", lambda v: finite(v.astype(np.float32)), "a finite baseline")
    rounds = _check_count(search_rounds, "search_rounds")
    points = _check_count(search_points, "search_points")
    cap = _check_count(max_workspace_bytes, "max_workspace_bytes")
    if noise is None and T < MIN_NOISE_FRAMES:
        raise ValueError("the noise level cannot be estimated from {} frames (the Welch window is {}): pass "
                         "noise=".format(T, MIN_NOISE_FRAMES))
    if g is None and T <= order.estimate_frames:
        raise ValueError("the decay cannot be estimated from {} frames: pass g=".format(T))
    launch_plan(1, T, cap, p)
    return y, g, noise, lam, s_min.astype(np.float32), baseline.astype(np.float32), rounds, points, cap


# ---- device side ----------------------------------------------------------------------------------------------------
class _Solver:
    """The traces, their parameters and tables on the device, and ``solve``: batches of (trace, penalty) problems through
    pmd_oasis_ar1 (p = 2: pmd_oasis_ar2) in the launches of launch_plan."""

    def __init__(self, ctx, Y, g, s_min, b, cap, largest, p=1):
        import torch

        self.ctx, self.Y, self.cap, self.p, self.order = ctx, Y, cap, p, _check_order(p)
        self.T, self.K = (int(x) for x in Y.shape)
        self.g, self.s_min, self.b = g, s_min, b
        self.pw = torch.from_numpy(self.order.tables(g, self.T)).to(ctx.device)
        n = max(p1 - p0 for p0, p1 in launch_plan(largest, self.T, cap, p))
        self.ws = torch.empty(workspace_bytes(self.T, n, p), dtype=torch.uint8, device=ctx.device)

    def solve(self, idx, lam, C=None, S=None, pools=False):
        """rss (float64) of the problems (trace idx[i], penalty lam[i]); with ``C`` / ``S`` ((T, n) device tensors) the
        calcium and spikes of problem i go to column i; with ``pools`` returns (rss, n_pools)."""
        import ctypes
        import torch
        from ._lib import ptr

        ctx, T, order = self.ctx, self.T, self.order
        idx = np.asarray(idx, dtype=np.int64)
        lam = np.asarray(lam, dtype=np.float32)
        n = len(idx)
        if n == 0 or idx.min() < 0 or idx.max() >= self.K:
            raise ValueError("problems must name traces 0 .. {}".format(self.K - 1))
        par = np.stack(order.par(self.g[idx], lam, self.s_min[idx], self.b[idx]), axis=1).astype(np.float32)
        rss, n_pools = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.int32)
        at = lambda t, p0: None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * p0)   # noqa: E731
        for p0, p1 in launch_plan(n, T, self.cap, self.p):
            col = torch.from_numpy(idx[p0:p1].astype(np.int32)).to(ctx.device)
            row = col if order.rows == 1 else torch.from_numpy((order.rows * idx[p0:p1]).astype(np.int32)).to(ctx.device)
            pr = torch.from_numpy(np.ascontiguousarray(par[p0:p1])).to(ctx.device)
            r = torch.empty(p1 - p0, dtype=torch.float64, device=ctx.device)
            npl = torch.empty(p1 - p0, dtype=torch.int32, device=ctx.device) if pools else None
            ctx.call(order.entry, ptr(self.Y), self.K, T, p1 - p0, ptr(col), ptr(pr), ptr(row), ptr(self.pw), order.ldtab(T),
                     at(C, p0), n, at(S, p0), n, ptr(r), ptr(npl), ptr(self.ws), self.ws.numel())
            rss[p0:p1] = r.cpu().numpy()
            if pools:
                n_pools[p0:p1] = npl.cpu().numpy()
        return (rss, n_pools) if pools else rss


def _device_noise(ctx, Y):
    """The Welch noise level of every column of the (T, K) device matrix (pmd_stats, 1024-frame chunks), float64."""
    import torch
    from ._lib import ptr

    T, K = (int(x) for x in Y.shape)
    mean = torch.empty(K, dtype=torch.float32, device=ctx.device)
    std = torch.empty(K, dtype=torch.float32, device=ctx.device)
    ws = torch.empty(ctx.lib.pmd_stats_workspace_bytes(T, K, 1024), dtype=torch.uint8, device=ctx.device)
    ctx.call("pmd_stats", ptr(Y), T, K, 1024, 1, ptr(mean), ptr(std), ptr(ws), ws.numel())
    ctx.sync()
    return std.cpu().numpy().astype(np.float64)


# ---- public entry point --------------------------------------------------------------------------------------------
def deconvolve(traces, g=None, noise=None, lam=None, s_min=0.0, baseline=0.0, search_rounds=5, search_points=8,
               max_workspace_bytes=1 << 30, device=None, ctx=None, p=1):
    """Spike inference of the rows of ``traces`` ((K, T) numbers, all finite): a Deconvolved with the denoised
    ``calcium`` c and the ``spikes`` s >= 0 ((K, T) float32) of the AR(1) model ``c_t = g c_{t-1} + s_t``,
    ``y = c + baseline + noise``, solved by OASIS on the device.

    ``p=2`` solves the AR(2) model ``c_t = g1 c_{t-1} + g2 c_{t-2} + s_t`` instead, whose response to a spike rises
    over several frames before it decays (slow indicators).  ``g`` is then a pair ``(g1, g2)`` or a (K, 2) array with
    real roots ``0 <= r <= d < 1`` of ``z^2 - g1 z - g2`` (``ar2_from_roots``, ``ar2_from_time_constants``), checked on
    the fp32 values; ``g=None`` estimates it (``estimate_ar2``, needs T > 11).  The solver pools greedily (Friedrich,
    Zhou & Paninski 2017, Alg. 3): on planted traces its objective lay within 0.4 % of the optimum for the roots
    (0.9, 0.3), 1.1 % for (0.95, 0.5) and 4.5 % for (0.97, 0.8), and it equals the optimum for ``g2 = 0``.
    ``Deconvolved.g`` is (K, 2); pool stacks take 24 T bytes per problem and the tables 12 K (T + 2) bytes.  With ``p=1``
    (the default) nothing differs from a call without ``p``.

    ``g`` (0 <= g < 1), ``noise`` (> 0), ``lam`` (>= 0), ``s_min`` (>= 0) and ``baseline`` are scalars or (K,) arrays.
    ``noise=None`` estimates the noise level of every trace as the decomposition does for a pixel (Welch, the upper half
    of the band; needs T >= 256, and reads high when fast transients put power there).  ``g=None`` estimates the decay
    from the autocovariances (estimate_decay).  ``lam=None`` searches the largest penalty whose residual sum of squares
    stays within ``noise^2 T``: round 0 and ``search_rounds`` rounds of ``search_points`` candidates per trace
    (search_lambda), then one solve per trace at the penalty found.  ``s_min > 0`` also merges every spike below it into
    its predecessor's pool.  The result reports what was used (``g``, ``noise``, ``lam``, ``baseline``), ``rss``,
    ``n_pools`` and the solves each trace took (``evaluations``).

    Device memory is 12 K T + 4 K (T + 1) bytes resident plus pool stacks of 12 T bytes per problem in flight, capped at
    ``max_workspace_bytes`` (deconvolve_device_bytes); a plan that does not fit raises ValueError.  No output bit
    depends on the cap.  Argument errors are raised before any device work."""
    import torch
    y, g, noise, lam, s_min, b, rounds, points, cap = check_arguments(
        traces, g, noise, lam, s_min, baseline, search_rounds, search_points, max_workspace_bytes, p)
    K, T = y.shape
    largest = K if lam is not None else K * max(2, points)
    with device_context(None, device, ctx) as (ctx, _):
        stats_bytes = 0 if noise is not None else int(ctx.lib.pmd_stats_workspace_bytes(T, K, 1024)) + 8 * K
        need = deconvolve_device_bytes(K=K, T=T, problems=largest, max_workspace_bytes=cap, stats_bytes=stats_bytes, p=p)
        check_fit(need, _device_free_bytes(ctx.device))
        Y = torch.from_numpy(y.T.copy()).to(ctx.device)      # frames-first, as every trace consumer here
        if noise is None:
            noise = _device_noise(ctx, Y)
        if g is None:
            g = _check_order(p).estimate(y, noise)
        g32 = g.astype(np.float32)
        solver = _Solver(ctx, Y, g32, s_min, b, cap, largest, p)
        every = np.arange(K, dtype=np.int64)
        if lam is None:
            lam32, evaluations = search_lambda(solver.solve, noise ** 2 * T, lambda_ceiling(y, g32, b), rounds, points)
        else:
            lam32, evaluations = lam.astype(np.float32), np.zeros(K, dtype=np.int64)
        C = torch.empty((T, K), dtype=torch.float32, device=ctx.device)
        S = torch.empty((T, K), dtype=torch.float32, device=ctx.device)
        rss, n_pools = solver.solve(every, lam32, C, S, pools=True)
        ctx.sync()
        calcium, spikes = np.ascontiguousarray(C.cpu().numpy().T), np.ascontiguousarray(S.cpu().numpy().T)
    return Deconvolved(calcium, spikes, g32, noise, lam32, b, rss, n_pools, evaluations + 1)
