"""The offset arithmetic of tests/bigbuf.py (no GPU): every geometry's live and alias windows lie in the buffer and are pairwise
disjoint, and its last window really starts past 2^31 elements, so the device tests built on it test what they claim to."""
import pytest

from tests import bigbuf as B


@pytest.mark.parametrize("name", sorted(B.GEOMETRIES))
def test_windows_lie_in_the_buffer_and_are_disjoint(name):
    g = B.GEOMETRIES[name]
    assert g.name == name
    live, alias = B.live_windows(g), B.alias_windows(g)
    assert len(live) == len(g.starts) and alias, "a geometry without an alias window tests nothing"
    windows = sorted(live + alias)
    assert windows[0][0] >= 0 and windows[-1][1] <= B.capacity(g.itemsize)
    for (a0, a1), (b0, b1) in zip(windows, windows[1:]):
        assert a1 - a0 == g.live and a1 <= b0, (name, (a0, a1), (b0, b1))


@pytest.mark.parametrize("name", sorted(B.GEOMETRIES))
def test_last_window_starts_past_2_to_the_31_elements(name):
    g = B.GEOMETRIES[name]
    assert max(g.starts) == g.starts[-1] >= 2 ** 31
    assert g.starts[-1] * g.itemsize >= 2 ** 32


def test_float32_rows_pass_2_to_the_32_bytes_at_row_one():
    g = B.GEOMETRIES["rows_f32"]
    assert g.starts == (0, 2 ** 30 + 4099, 2 ** 31 + 8198)
    assert g.starts[1] * 4 >= 2 ** 32 > g.starts[1]


def test_alias_windows_of_the_row_geometry():
    """Row 1 of a float32 view aliases through its byte offset only, row 2 through every truncation."""
    assert B.alias_windows(B.GEOMETRIES["rows_f32"]) == [(4099, 4099 + 70), (8198, 8198 + 70)]
    assert B.alias_windows(B.GEOMETRIES["rows_u16"]) == [(8198, 8198 + 70)]


def test_buffer_size():
    assert B.WORDS * 4 == (2 ** 31 + 2 ** 14) * 4 and B.capacity(2) == 2 * B.capacity(4)
