"""Host side of the one-pass fit diagnostics (localmd_amd.diagnostic_images.make_pmd_diagnostic_images): argument checks
before any device work, the batch plan, and the device-memory estimate.  No device needed."""
import numpy as np
import pytest
import scipy.sparse

import localmd_amd
from localmd_amd import _lib
from localmd_amd import diagnostic_images as DI
from localmd_amd.pmdarray import PMDArray


def _pmd(T=300, d1=6, d2=7, rank=3, order="F"):
    rng = np.random.default_rng(0)
    D = d1 * d2
    u = scipy.sparse.random(D, 4, density=0.5, random_state=1, format="coo")
    return PMDArray(u, rng.standard_normal((4, rank)), np.ones(rank), rng.standard_normal((rank, T)), (T, d1, d2), order,
                    rng.standard_normal((d1, d2)), np.ones((d1, d2)))


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a device context fails the test: the checks must come first."""
    def refuse(*a, **k):
        raise AssertionError("a device context was opened before the argument checks")
    monkeypatch.setattr(_lib.Context, "__init__", refuse)


def test_reexported():
    from localmd_amd import diagnostic_plots

    assert localmd_amd.make_pmd_diagnostic_images is DI.make_pmd_diagnostic_images
    assert diagnostic_plots.make_pmd_diagnostic_images is DI.make_pmd_diagnostic_images
    assert DI.PMDDiagnostics._fields[:4] == ("correlation", "autocorrelation", "pmd_correlation", "residual_correlation")
    assert DI.PMDDiagnostics._fields[4:] == ("residual_std", "explained_variance", "frame_residual_rms")


def test_pmd_must_be_a_pmdarray(no_device):
    mov = np.zeros((300, 6, 7), np.float32)
    with pytest.raises(TypeError):
        DI.make_pmd_diagnostic_images(mov, mov)
    with pytest.raises(TypeError):
        DI.make_pmd_diagnostic_images(mov, None)


@pytest.mark.parametrize("shape", [(299, 6, 7), (300, 7, 6), (300, 6, 8)])
def test_shape_mismatch(no_device, shape):
    with pytest.raises(ValueError, match="shape"):
        DI.make_pmd_diagnostic_images(np.zeros(shape, np.float32), _pmd())


@pytest.mark.parametrize("lag", [0, -1, 300, 301, 1.5])
def test_bad_lag(no_device, lag):
    with pytest.raises(ValueError, match="lag"):
        DI.make_pmd_diagnostic_images(np.zeros((300, 6, 7), np.float32), _pmd(), lag=lag)


@pytest.mark.parametrize("mode", ["median", "", None])
def test_bad_mode(no_device, mode):
    with pytest.raises(ValueError, match="mode"):
        DI.make_pmd_diagnostic_images(np.zeros((300, 6, 7), np.float32), _pmd(), mode=mode)


@pytest.mark.parametrize("T", [2, 1000, 1024, 1025, 2500, 5000, 20000])
@pytest.mark.parametrize("fbs", [1, 1024, 2047, 2048, 3000, 10000, 10 ** 6])
def test_batch_plan(T, fbs):
    plan = DI.diag_plan(T, fbs)
    nb = max(1024, fbs // 1024 * 1024)
    assert [(b0, b1) for b0, b1, _ in plan] == [(t, min(T, t + nb)) for t in range(0, T, nb)]
    covered = []
    for b0, b1, blocks in plan:
        assert b0 % 1024 == 0
        assert blocks[0][0] == b0 and blocks[-1][1] == b1
        for c0, c1 in blocks:
            assert c0 % DI.DIAG_FRAME_BLOCK == 0 and 0 < c1 - c0 <= DI.DIAG_RECON_FRAMES
            covered.append((c0, c1))
    assert covered[0][0] == 0 and covered[-1][1] == T
    assert all(a[1] == b[0] for a, b in zip(covered, covered[1:]))


def test_fused_workspace_matches_library():
    lib = _lib.load()
    for n, D in ((1, 1), (511, 42), (512, 1760), (2048, 262144), (1500, 16384)):
        assert DI._fused_workspace_bytes(n, D) == lib.pmd_diag_fused_workspace_bytes(n, D)
    assert lib.pmd_diag_fused_workspace_bytes(0, 100) == 0


def test_device_estimate_does_not_grow_with_T():
    D, n_cols, rank, nnz = 512 * 512, 54604, 3000, 4_000_000
    got = set()
    for T in (10_000, 40_000, 10 ** 6):
        plan = DI.diag_plan(T, 10000)
        nb = plan[0][1] - plan[0][0]
        got.add(DI._diag_device_bytes(D, nb, 4, n_cols, rank, nnz, 1, len(plan), True, False))
    assert len(got) == 1
    need, ring = got.pop()
    assert ring == 4 * D
    # two fp32 batches of 9216 frames dominate; the reconstruction block holds 2048 frames
    assert 2 * 9216 * D * 4 < need < 2 * 9216 * D * 4 + 4 * 2048 * D * 4 + 2048 * D * 8
    # the ring grows with lag and its element size; a single batch needs none
    n2, r2 = DI._diag_device_bytes(D, 9216, 2, n_cols, rank, nnz, 100, 3, True, False)
    assert r2 == 100 * D * 2
    assert DI._diag_device_bytes(D, 9216, 2, n_cols, rank, nnz, 100, 1, True, False)[1] == 0
    # factors already on the device are not counted again
    assert DI._diag_device_bytes(D, 9216, 4, n_cols, rank, nnz, 1, 3, True, True)[0] < need


def test_fit_check_names_lag():
    DI._check_fit(100, 40, 100, 7)
    with pytest.raises(ValueError, match="lag = 7"):
        DI._check_fit(100, 40, 80, 7)
    with pytest.raises(ValueError, match="frame_batch_size"):
        DI._check_fit(100, 40, 50, 7)
