"""
The float64 references of tests/prep_ref.py against independent implementations, on the CPU: the Welch restatement against
scipy.signal.welch, the chunked statistics against the fp32 oracle's loader.  This fixes the chunk semantics the GPU tests
rely on: a last chunk of 255 frames is not counted, one of 256 is.
"""
import numpy as np
import pytest

from localmd_amd.synthetic import make_movie
from oracle import pmd_oracle as O, philox
from tests import prep_ref as R

D1, D2 = 9, 13
LENGTHS = [256, 1279, 1280, 2100]


def _movie(T, offset):
    return (make_movie(T, D1, D2, seed=3) + np.float32(offset)).astype(np.float32)


def _scipy_stats(mov, frame_const=1024):
    """The same chunk rule with scipy's Welch inside."""
    from scipy.signal import welch

    y = mov.reshape(mov.shape[0], -1).astype(np.float64)
    T = y.shape[0]
    sig = []
    for t0 in range(0, T, frame_const):
        chunk = y[t0:t0 + frame_const]
        if chunk.shape[0] >= 256:
            _, pxx = welch(chunk.T, fs=1.0, window="hann", nperseg=256, noverlap=128, detrend="constant",
                           return_onesided=True, scaling="density", axis=-1)
            sig.append(np.sqrt(pxx[:, 65:129].mean(axis=1) / 2.0))
    return y.sum(axis=0) / T, np.mean(sig, axis=0)


@pytest.mark.parametrize("offset", [0, 30000])
@pytest.mark.parametrize("T", LENGTHS)
def test_stats_ref_against_scipy_welch(T, offset):
    """Two float64 implementations of one definition: they differ by rounding of the FFT alone (1e-11 relative leaves three
    decades over the 2^-53 per-operation error of a 256-point transform and a 64-bin mean)."""
    mov = _movie(T, offset)
    mean, sigma = R.stats_ref(mov, 1024, True)
    mean_s, sigma_s = _scipy_stats(mov)
    np.testing.assert_allclose(mean, mean_s, rtol=1e-14)
    np.testing.assert_allclose(sigma, sigma_s, rtol=1e-11)


@pytest.mark.parametrize("offset", [0, 30000])
@pytest.mark.parametrize("T", LENGTHS)
def test_stats_ref_against_the_oracle_loader(T, offset):
    """The oracle works in fp32.  Mean: a pairwise fp32 sum of up to 1024 frames per chunk, three chunk additions and a
    division, below 64 half-ulps = 3.8e-6 relative.  Sigma: fp32 detrend, window, 8 butterfly stages and the band mean, a few
    tens of roundings of 6e-8 that the square root halves: 2e-6 relative.  (Measured: 1.3e-6 and 1.5e-7.)"""
    mov = _movie(T, offset)
    mean, sigma = R.stats_ref(mov, 1024, True)
    np.random.seed(0)
    loader = O.PMDLoader(mov, philox.PhiloxSource(0), background_rank=0, compute_normalizer=True)
    assert loader.frame_constant == 1024
    em = np.abs(loader.mean_img.reshape(-1) - mean).max() / np.abs(mean).max()
    es = (np.abs(loader.std_img.reshape(-1) - sigma) / sigma).max()
    print(f"T={T} offset={offset}: oracle vs fp64 mean {em:.3g} sigma {es:.3g}")
    assert em <= 64 * 2.0 ** -24
    assert es <= 2e-6


def test_chunk_of_255_frames_is_not_counted_and_256_is():
    mov = _movie(1280, 0)
    y = mov.reshape(1280, -1).astype(np.float64)
    first = R.noise_sigma_ref(y[:1024].T)
    last = R.noise_sigma_ref(y[1024:1280].T)
    _, s1279 = R.stats_ref(mov[:1279], 1024, True)
    _, s1280 = R.stats_ref(mov, 1024, True)
    np.testing.assert_array_equal(s1279, first)
    np.testing.assert_allclose(s1280, 0.5 * (first + last), rtol=1e-15)
    assert np.abs(s1280 - s1279).max() > 1e-4      # the two rules are far apart on this movie


def test_stats_ref_degenerate_rules():
    mov = _movie(700, 0)
    for args in [(mov[:255], 1024, True), (mov, 1024, False), (mov, 128, True)]:
        _, sigma = R.stats_ref(*args)
        assert np.all(sigma == 1.0)
    const = mov.copy()
    const[:, 2, 5] = 517.25
    mean, sigma = R.stats_ref(const, 1024, True)
    c = 2 * D2 + 5
    assert sigma[c] == 1.0 and mean[c] == 517.25
    assert np.all(np.delete(sigma, c) != 1.0)


def test_frame_const_changes_the_chunks():
    mov = _movie(1300, 0)
    y = mov.reshape(1300, -1).astype(np.float64)
    _, s512 = R.stats_ref(mov, 512, True)
    want = (R.noise_sigma_ref(y[:512].T) + R.noise_sigma_ref(y[512:1024].T) + R.noise_sigma_ref(y[1024:].T)) / 3
    np.testing.assert_allclose(s512, want, rtol=1e-15)
    _, s1024 = R.stats_ref(mov, 1024, True)
    assert np.abs(s512 - s1024).max() > 1e-4


def test_one_line_references():
    rng = np.random.default_rng(0)
    D, nf, K = 7, 5, 3
    y = rng.standard_normal((nf, D)).astype(np.float32)
    mu, sd = rng.standard_normal(D).astype(np.float32), (1 + rng.random(D)).astype(np.float32)
    x = R.standardize_ref(y, mu, sd)
    assert x.shape == (D, nf) and x.dtype == np.float64
    assert x[3, 2] == (float(y[2, 3]) - float(mu[3])) / float(sd[3])
    b = np.linalg.qr(rng.standard_normal((D, K)))[0].astype(np.float32)
    pj = rng.standard_normal((K, nf)).astype(np.float32)
    assert np.array_equal(R.project_ref(b, x), b.astype(np.float64).T @ x)
    assert np.array_equal(R.filter_ref(x, b, pj), x - b.astype(np.float64) @ pj.astype(np.float64))
    assert np.all(R.filter_bound(x, b, pj, K) >= 7 * 2.0 ** -24 * np.abs(x))
    assert np.array_equal(R.scale_rows_ref(x, sd), x * sd.astype(np.float64)[:, None])


def test_rsvd_ref_is_exact_on_a_low_rank_input_and_matches_the_oracle():
    rng = np.random.default_rng(1)
    D, n, K = 60, 40, 3
    u = np.linalg.qr(rng.standard_normal((D, 5)))[0]
    v = np.linalg.qr(rng.standard_normal((n, 5)))[0]
    x = (u * (10.0 * 0.5 ** np.arange(5))) @ v.T
    om = rng.standard_normal((n, K + 10))
    b, s, sv = R.rsvd_ref(x, om, K)
    assert R.column_distance(b, u[:, :K]) < 1e-12
    np.testing.assert_allclose(s, 10.0 * 0.5 ** np.arange(K), rtol=1e-12)
    np.testing.assert_allclose(b @ sv, (u[:, :K] * (10.0 * 0.5 ** np.arange(K))) @ v[:, :K].T, atol=1e-12)
    ob, _ = O.loader_truncated_random_svd(x.astype(np.float32), om.astype(np.float32), K)
    assert R.column_distance(ob, b) < 1e-5


def test_sim_ref_tells_rows_from_columns():
    """A tile that is rough down its columns only: the spatial statistic of the (b1, b2) image differs from the one a
    b1 / b2 swap would give, so the non-square cases of the GPU test catch such a swap."""
    rng = np.random.default_rng(2)
    b1, b2, t = 6, 4, 30
    noise = rng.standard_normal((b1, b2, t))
    om = rng.standard_normal((t, 11))
    sp, tp = R.sim_ref(noise, om)
    u, _, sv = R.rsvd_ref(np.reshape(noise, (b1 * b2, t), order="F"), om, 1)
    assert sp == float(O.spatial_roughness_stat(u[:, 0].reshape((b1, b2), order="F")))
    assert tp == float(O.temporal_roughness_stat(sv[0]))
    swapped = float(O.spatial_roughness_stat(u[:, 0].reshape((b2, b1), order="F")))
    assert abs(swapped - sp) > 1e-3 * sp
