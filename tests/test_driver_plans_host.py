"""
Host-only planning of the decomposition driver: which tiles and pixels a rank works on (parallel.ownership_plan),
which frames are fitted and in which temporal windows (grid.select_frames, grid.temporal_windows), and the tile
batches (grid.tile_batches).  Expected values restate the reference's rules (localmd/decomposition.py:678-693 frame
selection, :528-569 the window draw, :757-774 rank cap and crop, :455-463 windows of windowed_pmd) in this file.
"""
import math

import numpy as np
import pytest

from localmd_amd import grid
from localmd_amd.parallel import ownership_plan, tile_partition

FOVS = [((512, 512), (20, 20)), ((60, 80), (20, 20)), ((70, 300), (10, 10)), ((96, 64), (32, 16))]


@pytest.mark.parametrize("fov,blocks", FOVS)
@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_ownership_plan_partitions_tiles_and_pixels(fov, blocks, world):
    d1, d2 = fov
    D = d1 * d2
    o1, o2 = grid.tile_origins(fov, list(blocks))
    n_tiles = len(o1) * len(o2)
    pix_c, _ = grid.tile_pixel_lists(fov, list(blocks), o1, o2)
    if world > len(o1):
        with pytest.raises(ValueError, match="distributed=True needs at least one tile row per rank"):
            ownership_plan(fov, blocks, world, 0)
        return
    plans = [ownership_plan(fov, blocks, world, r) for r in range(world)]
    # tile runs: the same list on every rank, a partition of range(n_tiles) into bands of whole tile rows
    for r, p in enumerate(plans):
        assert (p.world, p.rank, p.enabled) == (world, r, world > 1)
        assert p.runs == plans[0].runs and p.owned == plans[0].owned
        assert (p.t_lo, p.t_hi) == p.runs[r] and (p.O_lo, p.O_hi) == p.owned[r]
        assert (p.P_lo, p.P_hi) == (p.i_lo * d2, p.i_hi * d2)
    runs = plans[0].runs
    assert runs[0][0] == 0 and runs[-1][1] == n_tiles
    assert all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
    assert all(lo % len(o2) == 0 and hi % len(o2) == 0 and hi > lo for lo, hi in runs)
    assert [(lo // len(o2), hi // len(o2)) for lo, hi in runs] == tile_partition(len(o1), world)
    # owned ranges partition [0, D) in order
    owned = plans[0].owned
    assert owned[0][0] == 0 and owned[-1][1] == D
    assert all(a[1] == b[0] for a, b in zip(owned, owned[1:])) and all(hi > lo for lo, hi in owned)
    for p in plans:
        # every pixel of the rank's tiles lies in its slab, and it owns a part of its slab
        mine = pix_c[p.t_lo:p.t_hi]
        assert mine.min() >= p.P_lo and mine.max() < p.P_hi
        assert p.P_lo <= p.O_lo < p.O_hi <= p.P_hi
        assert 0 <= p.i_lo < p.i_hi <= d1
    if world == 1:
        assert (plans[0].P_lo, plans[0].P_hi) == (0, D) and (plans[0].O_lo, plans[0].O_hi) == (0, D)
        assert runs == [(0, n_tiles)]


def test_ownership_plan_slab_is_the_rows_of_the_band():
    # 60 x 80, 20 x 20 blocks: tile rows start at 0, 10, 20, 30, 40 (stride 10); two ranks get rows (0..2) and (3..4)
    a, b = (ownership_plan((60, 80), (20, 20), 2, r) for r in range(2))
    assert (a.i_lo, a.i_hi) == (0, 40) and (b.i_lo, b.i_hi) == (30, 60)
    assert a.owned == [(0, 30 * 80), (30 * 80, 60 * 80)]
    # blocks larger than the field of view are clamped first: one tile row, so a second rank has nothing to do
    assert ownership_plan((60, 80), (100, 100), 1, 0).runs == [(0, 1)]
    with pytest.raises(ValueError, match="1 rows, 2 ranks"):
        ownership_plan((60, 80), (100, 100), 2, 1)
    with pytest.raises(ValueError, match="block dimensions was less than"):
        ownership_plan((60, 80), (5, 20), 1, 0)


def _reference_frames(T, frame_range, window_chunks):
    """decomposition.py:678-693 with identify_window_chunks (:528-569) written out; draws from np.random."""
    if window_chunks is None:
        window_chunks = frame_range
    if T < frame_range:
        frame_range = T
        frames = [i for i in range(0, T)]
        if frame_range <= window_chunks:
            window_chunks = frame_range
        return frames, frame_range, window_chunks
    if frame_range <= window_chunks:
        window_chunks = frame_range
    num_intervals = math.ceil(frame_range / window_chunks)
    available = np.arange(0, T, window_chunks)
    if available[-1] > T - window_chunks:
        available[-1] = T - window_chunks
    starts = np.sort(np.random.choice(available, size=num_intervals, replace=False))
    frames = []
    for k in starts:
        frames.extend(range(int(k), int(min(k + window_chunks, T))))
    return frames, frame_range, window_chunks


def _reference_windows(n_frames, window_chunks, temporal_avg_factor, max_components):
    """decomposition.py:757-774 (rank cap, crop) and :455-463 (windows) written out."""
    if temporal_avg_factor >= n_frames:
        raise ValueError("Need at least {} frames".format(temporal_avg_factor))
    if n_frames // temporal_avg_factor <= max_components:
        max_components = int(n_frames // temporal_avg_factor)
    window_range = (n_frames // temporal_avg_factor) * temporal_avg_factor
    window_length = window_chunks
    if window_length > window_range:
        window_length = window_range
    start_points = list(range(0, window_range, window_length))
    if len(start_points) > 0 and start_points[-1] + window_length > window_range:
        start_points[-1] = window_range - window_length
    return max_components, window_range, window_length, start_points


PLANS = [
    # T, frame_range, window_chunks, temporal_avg_factor, max_components
    (400, 400, None, 10, 6),        # every frame, one window
    (300, 1000, None, 10, 50),      # T < frame_range: all frames, with the warning
    (300, 1000, 100, 10, 8),        # ... and several windows
    (1000, 400, 100, 10, 20),       # a drawn subset, four windows
    (1000, 400, 150, 10, 20),       # frame_range not a multiple of window_chunks: three chunks of 150 are drawn
    (997, 300, None, 7, 50),        # frames % temporal_avg_factor != 0 (crop < frames), rank cap lowered
    (205, 500, 50, 10, 5),          # crop = 200 = 4 windows of 50; the tail of 5 frames is cropped
    (250, 1000, 100, 10, 5),        # windows of 100 over crop = 250: the third is pulled back to 150
    (230, 230, 100, 10, 5),         # the drawn chunks themselves overlap (the last available start is pulled back)
]


@pytest.mark.parametrize("T,frame_range,window_chunks,taf,max_components", PLANS)
def test_frame_selection_and_windows_follow_the_reference(T, frame_range, window_chunks, taf, max_components):
    np.random.seed(1234)
    exp_frames, exp_range, exp_chunks = _reference_frames(T, frame_range, window_chunks)
    exp_state = np.random.get_state()
    said = []
    np.random.seed(1234)
    frames, fr, wc = grid.select_frames(T, frame_range, window_chunks, display=said.append)
    assert frames == exp_frames and (fr, wc) == (exp_range, exp_chunks)
    state = np.random.get_state()
    assert np.array_equal(state[1], exp_state[1]) and state[2] == exp_state[2]       # the same draws, no more
    assert said[-1] == "We are initializing on a total of {} frames".format(len(exp_frames))
    assert (said[0] == "WARNING: Specified using more frames than there are in the dataset.") == (T < frame_range)
    # `share` (the broadcast of rank 0's list) replaces a drawn list, and is not asked when nothing was drawn
    np.random.seed(1234)
    shared = grid.select_frames(T, frame_range, window_chunks, share=lambda fr_: list(range(len(fr_))))[0]
    assert shared == list(range(len(exp_frames)))

    exp = _reference_windows(len(exp_frames), exp_chunks, taf, max_components)
    said = []
    win = grid.temporal_windows(len(frames), wc, taf, max_components, display=said.append)
    assert (win.max_components, win.crop, win.win_len, win.win_starts) == exp and win.a_f == taf
    assert win.win_starts[-1] + win.win_len == win.crop and win.crop <= len(frames) < win.crop + taf
    assert (len(said) == 1 and said[0].startswith("WARNING: temporal avg factor is too big, max rank per block adjusted to "
                                                  + str(len(frames) // taf))) == (len(frames) // taf <= max_components)


def test_pulled_back_window_and_cropped_tail_values():
    win = grid.temporal_windows(230, 100, 10, 5)
    assert (win.crop, win.win_len, win.win_starts) == (230, 100, [0, 100, 130])
    win = grid.temporal_windows(205, 50, 10, 5)
    assert (win.crop, win.win_len, win.win_starts) == (200, 50, [0, 50, 100, 150])
    win = grid.temporal_windows(45, 45, 10, 50)
    assert (win.max_components, win.crop, win.win_len, win.win_starts) == (4, 40, 40, [0])


def test_window_plan_errors():
    with pytest.raises(ValueError, match="Need at least 10 frames"):
        grid.temporal_windows(10, 10, 10, 5)
    with pytest.raises(ValueError, match="window_chunks must be a multiple of temporal_avg_factor"):
        grid.temporal_windows(200, 45, 10, 5)
    grid.temporal_windows(200, 45, 15, 5)      # one window fewer frames than asked is no error: 195 = 4 x 45 + a pulled-back one


def test_tile_batches():
    assert grid.tile_batches(100, 1, 10, 1000) == [(0, 100)]
    assert grid.tile_batches(100, 1, 10, 300) == [(0, 30), (30, 60), (60, 90), (90, 100)]
    assert grid.tile_batches(100, 1, 10, 1) == [(lo, min(100, lo + 8)) for lo in range(0, 100, 8)]   # at least 8 tiles
    assert grid.tile_batches(100, 3, 10, 1) == [(0, 100)]      # several temporal windows: never batched
    assert grid.tile_batches(0, 1, 10, 1000) == [(0, 0)]       # a rank without tiles
