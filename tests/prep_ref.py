"""
Plain float64 NumPy references of the movie-preparation stage (test infrastructure only): what each entry point computes,
written for reading, with every input widened to float64 first.  tests/test_prep_ref.py pins the Welch restatement against
scipy.signal.welch and against the fp32 oracle; tests/test_gpu_prep_stage.py compares the HIP kernels with these.
"""
import numpy as np

NPERSEG = 256      # Welch window (periodic Hann), 50 % overlap
NOVERLAP = 128
MIN_FRAMES = 256   # a chunk (and a movie) shorter than this gives no noise estimate


def welch_ref(x):
    """One-sided Welch density of the rows of x (n, T >= 256): periodic Hann window of 256, overlap 128, constant detrend per
    segment, density scaling at fs = 1, mean over the (T - 128) // 128 full segments.  Returns (n, 129) float64."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[1]
    assert T >= NPERSEG
    step = NPERSEG - NOVERLAP
    nseg = (T - NOVERLAP) // step
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NPERSEG) / NPERSEG)
    scale = 1.0 / np.sum(win * win)
    acc = np.zeros((x.shape[0], NPERSEG // 2 + 1))
    for s in range(nseg):
        seg = x[:, s * step:s * step + NPERSEG]
        seg = (seg - seg.mean(axis=1, keepdims=True)) * win
        spec = np.fft.rfft(seg, axis=1)
        p = (spec.real ** 2 + spec.imag ** 2) * scale
        p[:, 1:-1] *= 2.0
        acc += p
    return acc / nseg


def noise_sigma_ref(x):
    """sqrt(mean(Pxx[65:129]) / 2) of the rows of x: the noise level read off the upper half band."""
    return np.sqrt(welch_ref(x)[:, 65:129].mean(axis=1) / 2.0)


def stats_ref(movie, frame_const=1024, compute_normalizer=True):
    """(mean, sigma) per pixel of a frames-first movie (T, ...), each of shape (D,).  The mean is the float64 sum over T.
    Sigma is the noise level of every chunk of frame_const frames that holds at least 256 frames (a shorter last chunk is
    not counted), averaged over the counted chunks; a sigma of exactly 0 becomes 1; with fewer than 256 frames in the
    movie, with the normaliser off, or with no chunk counted, every sigma is 1."""
    y = np.asarray(movie, dtype=np.float64)
    y = y.reshape(y.shape[0], -1)
    T, D = y.shape
    mean = y.sum(axis=0) / T
    sigma = np.ones(D)
    if not compute_normalizer or T < MIN_FRAMES:
        return mean, sigma
    total, counted = np.zeros(D), 0
    for t0 in range(0, T, frame_const):
        chunk = y[t0:t0 + frame_const]
        if chunk.shape[0] >= MIN_FRAMES:
            total += noise_sigma_ref(chunk.T)
            counted += 1
    if counted:
        sigma = total / counted
        sigma[sigma == 0] = 1.0
    return mean, sigma


def standardize_ref(y, mu, sd):
    """(y - mu) / sd, pixel-major: y (nf, D) frames first -> (D, nf)."""
    y, mu, sd = (np.asarray(a, dtype=np.float64) for a in (y, mu, sd))
    return ((y - mu[None, :]) / sd[None, :]).T


def project_ref(basis, x):
    """B^T X: basis (D, K), x (D, T) -> (K, T)."""
    return np.asarray(basis, dtype=np.float64).T @ np.asarray(x, dtype=np.float64)


def filter_ref(x, basis, pj):
    """X - B pj with the GIVEN pj (K, nf); it is not recomputed from x."""
    return np.asarray(x, dtype=np.float64) - np.asarray(basis, dtype=np.float64) @ np.asarray(pj, dtype=np.float64)


def filter_bound(x, basis, pj, K):
    """Elementwise error bound of the filter: one fma chain of K terms, one subtraction, one stored rounding per extra pass
    of 64 columns: (K + 4) 2^-24 (|x| + sum_k |b_k| |pj_k|)."""
    mag = np.abs(np.asarray(x, dtype=np.float64)) + np.abs(np.asarray(basis, dtype=np.float64)) @ np.abs(np.asarray(pj, dtype=np.float64))
    return (K + 4) * 2.0 ** -24 * mag


def scale_rows_ref(x, w):
    """x[c][f] * w[c]."""
    return np.asarray(x, dtype=np.float64) * np.asarray(w, dtype=np.float64)[:, None]


def rsvd_ref(x, omega, K):
    """Rank-K randomised SVD basis: q = qr(X Om), svd(q^T X), (q u)[:, :K].  Returns (basis (D, K), s (K,), s v (K, n))."""
    x, omega = np.asarray(x, dtype=np.float64), np.asarray(omega, dtype=np.float64)
    q, _ = np.linalg.qr(x @ omega)
    u, s, vt = np.linalg.svd(q.T @ x, full_matrices=False)
    return (q @ u)[:, :K], s[:K], s[:K, None] * vt[:K]


def column_distance(a, b):
    """Largest per-column L2 distance of a to b after flipping each column of a to the sign of its match in b."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    sgn = np.where(np.sum(a * b, axis=0) < 0, -1.0, 1.0)
    return float(np.sqrt(np.sum((a * sgn[None, :] - b) ** 2, axis=0)).max())


def sim_ref(noise, omega):
    """One iteration of the threshold simulation: the rank-1 rSVD of a noise tile (b1, b2, t) with sketch omega (t, 11),
    tile pixels in column-major order, then the (spatial, temporal) roughness of the spatial component and of s v."""
    from oracle import pmd_oracle as O

    noise = np.asarray(noise, dtype=np.float64)
    b1, b2, t = noise.shape
    u, _, sv = rsvd_ref(np.reshape(noise, (b1 * b2, t), order="F"), omega, 1)
    img = np.reshape(u[:, 0], (b1, b2), order="F")
    return float(O.spatial_roughness_stat(img)), float(O.temporal_roughness_stat(sv[0]))
