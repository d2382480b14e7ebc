"""
Host-side tests of what the movie consumers share around an expanded block: the panel code, the (d1, P, d2) pixel order
of a block of P panels, the walk over the reconstruction blocks of a batch, and the device bytes of the expander as a
term of every consumer's estimate.
"""
import numpy as np
import pytest

from localmd_amd import _expand as X
from localmd_amd import export as E
from localmd_amd import maps as MP
from localmd_amd import quantiles as Q
from localmd_amd import summary as SM
from localmd_amd import traces as TR
from localmd_amd._stream import BLOCK, batch_buffer_bytes, block_plan, block_walk, factor_bytes


def test_panel_code_two_bits_per_panel_first_panel_lowest():
    assert E._PANEL_CODE is X._PANEL_CODE and X._PANEL_CODE == {"raw": 0, "denoised": 1, "residual": 2}
    assert X.panel_code(("raw", "denoised", "residual")) == 0 | 1 << 2 | 2 << 4
    assert X.panel_code(("residual",)) == 2
    assert X.panel_code(("denoised", "residual")) == 1 | 2 << 2
    assert X.panel_code(()) == 0


# ---- the pixel order of a block of P panels --------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 3])
def test_interleave_places_panel_pixels_side_by_side(P):
    d1, d2 = 5, 7                                  # 35 pixels: no multiple of 64
    vecs = [np.arange(d1 * d2, dtype=np.float32) + 1000 * p for p in range(P)]
    got = X.interleave(vecs, d1, d2)
    assert got.shape == (P * d1 * d2,) and got.dtype == np.float32
    for p in range(P):
        for i in range(d1):
            for j in range(d2):
                assert got[i * P * d2 + p * d2 + j] == vecs[p][i * d2 + j]


@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("lead", [(), (3,), (2, 3)])
def test_split_panels_inverts_interleave(P, lead):
    d1, d2 = 5, 7
    rng = np.random.default_rng(P)
    per_panel = [rng.standard_normal(lead + (d1 * d2,)).astype(np.float32) for _ in range(P)]
    a = np.empty(lead + (P * d1 * d2,), dtype=np.float32)
    for idx in np.ndindex(*lead):
        a[idx] = X.interleave([v[idx] for v in per_panel], d1, d2)
    back = X.split_panels(a, d1, P, d2)
    assert len(back) == P
    for v, w in zip(per_panel, back):
        assert w.shape == lead + (d1 * d2,) and w.flags["C_CONTIGUOUS"] and np.array_equal(v, w)
    # and the other way round: interleaving the split vectors gives the block order back
    flat = a.reshape(-1, P * d1 * d2)[0]
    assert np.array_equal(X.interleave(X.split_panels(flat, d1, P, d2), d1, d2), flat)


# ---- the walk over the blocks of a batch -----------------------------------------------------------------------------
class _FakeBatch:
    def __init__(self, address, esize):
        self.address, self.esize = address, esize

    def data_ptr(self):
        return self.address

    def element_size(self):
        return self.esize


def test_block_walk_yields_the_blocks_of_the_plan():
    T, fbs, D, esize = 2500, 2048, 35, 2
    plan = block_plan(T, fbs)
    assert [(b0, b1) for b0, b1, _ in plan] == [(0, 2048), (2048, 2500)]
    walk = block_walk(plan, D)
    base = {0: 1 << 20, 2048: 1 << 30}
    seen = [(c0, m, yp.value) for b0, _, _ in plan for c0, m, yp in walk(_FakeBatch(base[b0], esize), b0)]
    want = [(c0, c1 - c0, base[b0] + (c0 - b0) * D * esize) for b0, _, blocks in plan for c0, c1 in blocks]
    assert seen == want
    assert [(c0, m) for c0, m, _ in seen] == [(0, 1024), (1024, 1024), (2048, 452)]
    assert [p - base[0] for _, _, p in seen[:2]] == [0, 1024 * D * esize] and seen[2][2] == base[2048]
    # without a movie there is no address, the blocks are the same
    assert [b for b0, _, _ in plan for b in walk(None, b0)] == [(c0, m, None) for c0, m, _ in want]


# ---- the expander's bytes as a term of every estimate ----------------------------------------------------------------
_SHAPE = dict(D=4099, n_cols=300, rank=12, n_entries=900, n_a=50000, n_patches=65)
_SRC = dict(nb=3072, esize=2, needs_movie=True, host_source=True, n_batches=3)
_BATCH = batch_buffer_bytes(3072, 4099, 2, True, 3)
_MIB = 1 << 20


def test_expander_bytes_terms():
    D, n_cols, rank = _SHAPE["D"], _SHAPE["n_cols"], _SHAPE["rank"]
    tables = 8 * 66 + 900 * (8 * 4 + 4 * 64) + 4 * 50000
    a = X.expander_bytes(factors_on_device=False, **_SHAPE)
    assert a == tables + 8 * D + 4 * rank * BLOCK + 4 * n_cols * rank + 4 * n_cols * BLOCK
    assert a - X.expander_bytes(factors_on_device=True, **_SHAPE) == 4 * n_cols * rank
    assert a - X.expander_bytes(factors_on_device=False, stats=False, **_SHAPE) == 8 * D
    assert a - X.expander_bytes(factors_on_device=False, own_ct=False, **_SHAPE) == 4 * n_cols * BLOCK
    assert X.expander_bytes(factors_on_device=False, block_panels=2, **_SHAPE) - a == 4 * 2 * BLOCK * D
    assert factor_bytes(n_cols, rank, False) == 4 * rank * BLOCK + 4 * n_cols * rank
    assert factor_bytes(n_cols, 0, False) == factor_bytes(0, rank, False) == 0
    with pytest.raises(TypeError):
        X.expander_bytes(D, n_cols, rank)               # keyword-only: no silent mis-ordering


def test_export_estimate_is_the_expander_plus_its_ring():
    got = E.export_device_bytes(_SHAPE["D"], 3072, 2, 3, 4, 300, 12, 900, 50000, 65, True, True, 3, True, False)
    ring = E.HOST_SLOTS * BLOCK * _SHAPE["D"] * 3 * 4
    assert got == X.expander_bytes(factors_on_device=False, **_SHAPE) + _BATCH + ring + _MIB


def test_maps_estimate_is_the_expander_plus_its_accumulators():
    D, K = _SHAPE["D"], 5
    got = MP.maps_device_bytes(K=K, n_acc=3, n_expand=2, factors_on_device=False, factor_sums=False, **_SHAPE, **_SRC)
    own = 8 * 3 * (K + 2) * D + 4 * K * BLOCK + 2 * 4 * D + 4 * 2 * D      # accumulators, regressors, mean + std, shift
    assert got == X.expander_bytes(factors_on_device=False, stats=False, block_panels=2, **_SHAPE) + own + _BATCH + _MIB
    # the denoised sums from the factors: the tables and factors, no coefficient block, no expanded block
    got = MP.maps_device_bytes(K=K, n_acc=1, n_expand=0, factors_on_device=False, factor_sums=True, **_SHAPE, **_SRC)
    own = 8 * (K + 2) * D + 4 * K * BLOCK + 2 * 4 * D + 16 * 12 * K + 4 * 300 * K + 4 * K * D + 4 * D
    assert got == X.expander_bytes(factors_on_device=False, stats=False, own_ct=False, **_SHAPE) + own + _BATCH + _MIB


def test_summary_estimate_is_the_expander_plus_its_state():
    D = _SHAPE["D"]
    got = SM.summary_device_bytes(n_raw=1, n_expand=2, need_ext=True, need_arg=True, need_mom=True,
                                  factors_on_device=False, **_SHAPE, **_SRC)
    own = (8 + 8 + 32 + 4) * 3 * D
    assert got == X.expander_bytes(factors_on_device=False, block_panels=2, **_SHAPE) + own + _BATCH + _MIB


def test_quantile_estimate_is_the_expander_plus_its_histograms():
    D = _SHAPE["D"]

    def state(N):
        return 3 * (4 * Q.BINS * Q.GROUP * (-(-N // Q.GROUP)) + 8 * N) + 4 * N

    got = Q.quantile_device_bytes(n_raw=1, n_expand=2, n_pos=3, centred=True, factors_on_device=False, **_SHAPE, **_SRC)
    own = state(D) + state(2 * D)
    assert got == X.expander_bytes(factors_on_device=False, block_panels=2, **_SHAPE) + own + _BATCH + _MIB


def test_traces_estimate_shares_the_factor_term():
    D, K, nb = _SHAPE["D"], 7, 3072
    got = TR.traces_device_bytes(D, nb, 2, K, 3, 0, 500, 9, 2, 4, 91, 300, 12, True, True, 3, False)
    own = (8 * 500 + 8 * (TR.SEG_FIELDS * 9 + TR.SPLIT_FIELDS * 2) + 4 * 4 * nb + 4 * K * nb * 6
           + 4 * (K * BLOCK + K * 12 + K) + 12 * 91 + 8 * (K + 1))
    assert got == factor_bytes(300, 12, False) + own + _BATCH + _MIB
