"""
_expand.KindPlan and _expand.KindBlocks, the two halves under summary_images, quantile_images, regressor_maps, superpixels
and the rolling baseline, driven on the host: the plan's facts and how often it builds the expand tables, and, with a
recording Expander and read_batches, the exact sequence of batch / coefficients / expand / each calls of the one walk and
their arguments.  No GPU.
"""
import numpy as np
import pytest
import scipy.sparse

from localmd_amd import _expand as X
from localmd_amd import export as E
from localmd_amd.baseline import baseline_device_bytes
from localmd_amd.maps import maps_device_bytes
from localmd_amd.pmdarray import PMDArray
from localmd_amd.quantiles import quantile_device_bytes
from localmd_amd.summary import summary_device_bytes
from localmd_amd.superpixels import superpixel_device_bytes

T, D1, D2 = 2500, 6, 7
D = D1 * D2
ESIZE = 2                                  # the movie is uint16
BLOCKS = [(0, 1024), (1024, 1024), (2048, 452)]
BATCHES = {1024: [(0, 1024), (1024, 2048), (2048, 2500)], 2048: [(0, 2048), (2048, 2500)]}
BLOCK_PTR = 0x7000000


def _pmd(T=T, rank=3):
    rng = np.random.default_rng(0)
    u = scipy.sparse.random(D, 4, density=0.5, random_state=1, format="coo")
    return PMDArray(u, rng.standard_normal((4, rank)), np.ones(rank), rng.standard_normal((rank, T)), (T, D1, D2), "F",
                    rng.standard_normal((D1, D2)), np.ones((D1, D2)))


def _movie(T=T):
    return np.zeros((T, D1, D2), np.uint16)


class _Tensor:
    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address

    def element_size(self):
        return ESIZE


def _base(b0):
    """The device address of the fake batch that starts at frame b0."""
    return 0x100000 * (1 + b0 // 1024)


@pytest.fixture
def rig(monkeypatch):
    """(log, built, blocks): blocks(raw, panels, fbs, **kw) is a KindBlocks on fakes that record into log; ``built``
    counts the calls of expand_tables_for."""
    log, built = [], []
    real_tables = E.expand_tables_for

    def tables(pmd):
        built.append(pmd)
        return real_tables(pmd)

    class _Expander:
        def __init__(self, ctx, pmd, dv, tabs, xt, *, own_ct=True, block_panels=0):
            assert tabs is not None and xt is not None
            log.append(("Expander", own_ct, block_panels))
            self.block = _Tensor(BLOCK_PTR) if block_panels else None

        def coefficients(self, c0, m):
            log.append(("coefficients", c0, m))

        def expand(self, n, n_panels, code, yp, elem):
            log.append(("expand", n, n_panels, code, None if yp is None else yp.value, elem))

    def read_batches(ctx, movie, batches, frame_batch_size, num_workers, consume):
        assert ctx == "ctx" and num_workers == 3
        assert batches == BATCHES[frame_batch_size]
        for b0, b1 in batches:
            if movie is None:
                consume(None, 0, b0, b1 - b0)
            else:
                consume(_Tensor(_base(b0)), 1, b0, b1 - b0)

    monkeypatch.setattr(E, "expand_tables_for", tables)
    monkeypatch.setattr(X, "Expander", _Expander)
    monkeypatch.setattr(X, "read_batches", read_batches)

    def blocks(raw, panels, fbs, **kw):
        pmd = _pmd()
        plan = X.KindPlan(pmd, _movie() if raw or "residual" in panels else None, raw=raw, panels=panels,
                          frame_batch_size=fbs)
        return X.KindBlocks("ctx", pmd, None, plan, 3, **kw)

    return log, built, blocks


def _each(log):
    def each(c0, m, yp, elem, xp):
        log.append(("each", c0, m, None if yp is None else yp.value, elem, None if xp is None else xp.value))

    return each


def _whole(log):
    def whole(Y, elem, b0, n):
        log.append(("batch", Y.value, elem, b0, n))

    return whole


def _yp(c0, fbs):
    b0 = c0 // fbs * fbs
    return _base(b0) + (c0 - b0) * D * ESIZE


@pytest.mark.parametrize("fbs", [1024, 2048])
def test_raw_only_walks_the_raw_frames_in_place_and_builds_no_tables_or_expander(rig, fbs):
    log, built, blocks = rig
    kb = blocks(True, (), fbs)
    assert kb.ex is None and built == [] and log == []
    kb.run(_each(log), batch=_whole(log))
    want = []
    for b0, b1 in BATCHES[fbs]:
        want.append(("batch", _base(b0), 1, b0, b1 - b0))
        want += [("each", c0, m, _yp(c0, fbs), 1, None) for c0, m in BLOCKS if b0 <= c0 < b1]
    assert log == want
    assert [e[3] for e in log if e[0] == "each"] == [_base(b0) + (c0 - b0) * D * ESIZE
                                                      for b0, b1 in BATCHES[fbs] for c0, _ in BLOCKS if b0 <= c0 < b1]


@pytest.mark.parametrize("fbs", [1024, 2048])
def test_panels_only_reads_no_movie_and_hands_the_expanded_block(rig, fbs):
    log, built, blocks = rig
    kb = blocks(False, ("denoised",), fbs)
    assert len(built) == 1 and log == [("Expander", True, 1)] and kb.plan.movie is None
    del log[:]
    kb.run(_each(log), batch=_whole(log))          # no movie: the batch callback is never called
    code = X.panel_code(("denoised",))
    want = []
    for c0, m in BLOCKS:
        want += [("coefficients", c0, m), ("expand", m, 1, code, None, 0), ("each", c0, m, None, 0, BLOCK_PTR)]
    assert log == want


@pytest.mark.parametrize("fbs", [1024, 2048])
def test_raw_and_two_panels_batch_then_per_block_product_expansion_and_each(rig, fbs):
    log, built, blocks = rig
    panels = ("denoised", "residual")
    kb = blocks(True, panels, fbs, own_ct=True)
    assert len(built) == 1 and log == [("Expander", True, 2)]
    del log[:]
    kb.run(_each(log), batch=_whole(log))
    code = X.panel_code(panels)
    want = []
    for b0, b1 in BATCHES[fbs]:
        want.append(("batch", _base(b0), 1, b0, b1 - b0))
        for c0, m in BLOCKS:
            if b0 <= c0 < b1:
                yp = _base(b0) + (c0 - b0) * D * ESIZE
                want += [("coefficients", c0, m), ("expand", m, 2, code, yp, 1), ("each", c0, m, yp, 1, BLOCK_PTR)]
    assert log == want
    del log[:]
    kb.run(_each(log))                             # without a batch callback: the same blocks
    assert log == [e for e in want if e[0] != "batch"]
    del log[:]
    # ``before`` gets the block's raw frames ahead of its product and expansion
    kb.run(_each(log), before=lambda c0, m, yp, elem: log.append(("before", c0, m, yp.value, elem)))
    ahead = []
    for e in want:
        if e[0] == "coefficients":
            ahead.append(("before", e[1], e[2], _yp(e[1], fbs), 1))
        if e[0] != "batch":
            ahead.append(e)
    assert log == ahead


@pytest.mark.parametrize("fbs", [1024, 2048])
def test_read_movie_false_runs_the_same_blocks_without_a_source(rig, fbs):
    log, _, blocks = rig
    kb = blocks(True, ("denoised",), fbs)
    del log[:]
    kb.run(_each(log), batch=_whole(log), read_movie=False)
    code = X.panel_code(("denoised",))
    want = []
    for c0, m in BLOCKS:
        want += [("coefficients", c0, m), ("expand", m, 1, code, None, 0), ("each", c0, m, None, 0, BLOCK_PTR)]
    assert log == want
    del log[:]
    kb.run(_each(log))                             # and the next pass reads the movie again
    assert [e for e in log if e[0] == "each"] == [("each", c0, m, _yp(c0, fbs), 1, BLOCK_PTR) for c0, m in BLOCKS]


def test_tables_are_built_once_when_forced_and_the_expander_can_go_without_a_block(rig):
    log, built, _ = rig
    pmd = _pmd()
    plan = X.KindPlan(pmd, _movie(), raw=True, panels=(), frame_batch_size=1024, tables=True)
    assert len(built) == 1 and plan.xt is not None and plan.reads_movie
    kb = X.KindBlocks("ctx", pmd, None, plan, 3, own_ct=False)
    assert log == [("Expander", False, 0)] and kb.ex is not None
    del log[:]
    kb.run(_each(log))
    assert log == [("each", c0, m, _yp(c0, 1024), 1, None) for c0, m in BLOCKS]


def test_a_decomposition_of_no_frames_has_no_blocks_and_builds_no_tables(rig):
    _, built, _ = rig
    plan = X.KindPlan(_pmd(T=0), None, raw=False, panels=("denoised",), frame_batch_size=1024)
    assert plan.T == 0 and plan.plan == [] and plan.nb == 0 and plan.xt is None and built == []


def test_a_movie_of_another_shape_is_refused_by_the_plan():
    with pytest.raises(ValueError, match="the movie has shape"):
        X.KindPlan(_pmd(), _movie(T - 1), raw=True, panels=(), frame_batch_size=1024)


def test_facts_are_the_keywords_written_out_by_hand_and_feed_every_device_bytes():
    pmd = _pmd(T=300)
    tabs, xt = E.expand_tables_for(pmd)
    plan = X.KindPlan(pmd, _movie(300), raw=True, panels=("denoised", "residual"), frame_batch_size=1024)
    assert (plan.T, plan.d1, plan.d2, plan.D) == (300, D1, D2, D) and plan.plan == [(0, 300, [(0, 300)])]
    assert (plan.on_device, plan.esize, plan.n_cols, plan.rank, plan.reads_movie) == (False, 2, 4, 3, True)
    by_hand = dict(D=42, nb=300, esize=2, n_cols=4, rank=3, n_entries=len(xt["entries"]), n_a=int(tabs["a"].size),
                   n_patches=1, host_source=True, n_batches=1, factors_on_device=False)
    assert len(xt["entries"]) > 0 and int(tabs["a"].size) > 0
    assert plan.facts(None) == by_hand
    assert plan.facts({"rs": None}) == dict(by_hand, factors_on_device=True)
    f = plan.facts(None)
    own = dict(n_raw=1, n_expand=2, need_ext=True, need_arg=True, need_mom=True, needs_movie=True)
    assert summary_device_bytes(**f, **own) == summary_device_bytes(**by_hand, **own)
    own = dict(n_raw=1, n_expand=2, n_pos=2, centred=True, needs_movie=True)
    assert quantile_device_bytes(**f, **own) == quantile_device_bytes(**by_hand, **own)
    own = dict(K=3, n_acc=3, n_expand=2, needs_movie=True, factor_sums=False)
    assert maps_device_bytes(**f, **own) == maps_device_bytes(**by_hand, **own)
    for kind in ("denoised", "raw"):
        own = dict(T=300, kind=kind, threshold_given=False)
        assert superpixel_device_bytes(**f, **own) == superpixel_device_bytes(**by_hand, **own)
        own = dict(T=300, temporal_bin=16, kind=kind, host_dest=True, method="maximin", half=3)
        assert baseline_device_bytes(**f, **own) == baseline_device_bytes(**by_hand, **own)
    # raw only: no tables, and the table terms are zero
    raw = X.KindPlan(pmd, _movie(300), raw=True, panels=(), frame_batch_size=1024)
    assert raw.facts(None) == dict(by_hand, n_entries=0, n_a=0, n_patches=0)
    # no movie given: a host source of 4-byte elements, as every consumer has assumed
    den = X.KindPlan(pmd, None, raw=False, panels=("denoised",), frame_batch_size=1024)
    assert (den.on_device, den.esize, den.reads_movie, den.movie) == (False, 4, False, None)
    assert den.facts(None) == dict(by_hand, esize=4)
