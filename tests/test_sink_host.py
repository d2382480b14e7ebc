"""
_sink.movie_pass, the one scaffold under export_movie, dff_movie and the two registrations, driven on the host with a
recording context, destination and sink: the order of open / finish / sync / shutdown / close on success, of sink.abort /
dest.abort / shutdown on every kind of failure, the block counter, and the pass without a destination.  No GPU.
"""
import os

import numpy as np
import pytest

from localmd_amd import _sink as S

BLOCKS = [(0, 1024), (1024, 1024), (2048, 17)]


class _Ctx:
    def __init__(self, log):
        self.log = log

    def sync(self):
        self.log.append("sync")


class _FakeDest:
    kind, target = "array", "the array"

    def __init__(self, log):
        self.log = log

    def open(self):
        self.log.append("open")

    def abort(self):
        self.log.append("dest.abort")

    def shutdown(self):
        self.log.append("shutdown")

    def close(self):
        self.log.append("close")
        return self.target


class _FakeSink:
    def __init__(self, log, fail_finish=None):
        self.log, self.fail_finish = log, fail_finish

    def dst(self, k, t0):
        self.log.append(("dst", k, t0))
        return 4096 * (k + 1)

    def done(self, k, t0, m):
        self.log.append(("done", k, t0, m))

    def finish(self):
        self.log.append("finish")
        if self.fail_finish is not None:
            raise self.fail_finish

    def abort(self):
        self.log.append("sink.abort")


def _blocks(each):
    for c0, m in BLOCKS:
        each(c0, m, "yp%d" % c0, 1)


@pytest.fixture
def rig(monkeypatch):
    """(log, ctx, dest, run): run(write, fail_finish=None) drives movie_pass over BLOCKS with the fakes."""
    log = []
    ctx, dest = _Ctx(log), _FakeDest(log)

    def run(write, fail_finish=None):
        def make(c, d, frame_shape, np_dtype, capacity):
            assert c is ctx and d is dest and tuple(frame_shape) == (5, 7) and np_dtype == np.float32 and capacity == 1024
            log.append("sink")
            return _FakeSink(log, fail_finish)

        monkeypatch.setattr(S, "_make_sink", make)
        return S.movie_pass(ctx, dest, (5, 7), np.dtype(np.float32), 1024, _blocks, write)

    return log, ctx, dest, run


_ABORTED = ["sink.abort", "dest.abort", "shutdown"]


def test_success_order_block_counter_and_return_value(rig):
    log, _, dest, run = rig

    def write(c0, m, yp, elem, out):
        log.append(("write", c0, m, yp, elem, out.value))

    assert run(write) is dest.target
    want = ["open", "sink"]
    for k, (c0, m) in enumerate(BLOCKS):
        want += [("dst", k, c0), ("write", c0, m, "yp%d" % c0, 1, 4096 * (k + 1)), ("done", k, c0, m)]
    assert log == want + ["finish", "sync", "shutdown", "close"]


@pytest.mark.parametrize("error", [RuntimeError("the kernel failed"), KeyboardInterrupt()])
def test_a_failing_second_block_aborts_in_order_and_raises_the_same_object(rig, error):
    log, _, _, run = rig

    def write(c0, m, yp, elem, out):
        if c0 == BLOCKS[1][0]:
            raise error

    with pytest.raises(type(error)) as got:
        run(write)
    assert got.value is error
    assert log == ["open", "sink", ("dst", 0, 0), ("done", 0, 0, 1024), ("dst", 1, 1024)] + _ABORTED
    assert "close" not in log and "finish" not in log and "sync" not in log


def test_a_writer_thread_error_in_finish_aborts_in_the_same_order(rig):
    log, _, _, run = rig
    error = OSError("disk full")
    with pytest.raises(OSError) as got:
        run(lambda c0, m, yp, elem, out: None, fail_finish=error)
    assert got.value is error
    assert log[-4:] == ["finish"] + _ABORTED and "close" not in log and "sync" not in log
    assert [e for e in log if isinstance(e, tuple) and e[0] == "done"] == [("done", k, c0, m)
                                                                          for k, (c0, m) in enumerate(BLOCKS)]


def test_a_failing_sink_construction_still_removes_the_file(rig, monkeypatch):
    log, ctx, dest, _ = rig

    def make(*a):
        raise MemoryError("no page-locked memory")

    monkeypatch.setattr(S, "_make_sink", make)
    with pytest.raises(MemoryError):
        S.movie_pass(ctx, dest, (5, 7), np.dtype(np.float32), 1024, _blocks, lambda *a: None)
    assert log == ["open", "dest.abort", "shutdown"]


def test_without_a_destination_every_block_is_seen_and_nothing_is_opened(monkeypatch):
    log = []
    monkeypatch.setattr(S, "_make_sink", lambda *a: pytest.fail("a sink was built without a destination"))
    seen = []
    res = S.movie_pass(_Ctx(log), None, (5, 7), np.dtype(np.float32), 1024, _blocks,
                       lambda c0, m, yp, elem, out: seen.append((c0, m, yp, elem, out)))
    assert res is None
    assert seen == [(c0, m, "yp%d" % c0, 1, None) for c0, m in BLOCKS]
    assert log == ["sync"]
    error = ValueError("bad block")

    def write(c0, m, yp, elem, out):
        raise error

    with pytest.raises(ValueError) as got:
        S.movie_pass(_Ctx(log), None, (5, 7), np.dtype(np.float32), 1024, _blocks, write)
    assert got.value is error and log == ["sync"]


def test_a_real_npy_destination_is_removed_when_the_second_block_fails(tmp_path, monkeypatch):
    path = str(tmp_path / "out.npy")
    dest = S._destination(path, (3, 5, 7), np.dtype(np.float32), None, 0)
    assert dest.kind == "npy"
    log = []
    monkeypatch.setattr(S, "_make_sink", lambda *a: _FakeSink(log))
    created = []

    def write(c0, m, yp, elem, out):
        created.append(os.path.exists(path))
        if c0:
            raise RuntimeError("the second block failed")

    with pytest.raises(RuntimeError, match="second block"):
        S.movie_pass(_Ctx(log), dest, (5, 7), np.dtype(np.float32), 2, lambda each: [each(0, 2, None, 0), each(2, 1, None, 0)],
                     write)
    assert created == [True, True] and not os.path.exists(path)
    assert dest.writer is None and dest.pool is None and "sink.abort" in log


def test_front_door_checks():
    class _C:
        device_index = 3

    class _P:
        _dev = {"ctx": _C()}

    assert S.device_index(None, None, None) == 0 and S.device_index(None, "2", None) == 2
    assert S.device_index(None, 1, _C()) == 3 and S.device_index(_P(), 1, None) == 3
    for ok in (None, True, False):
        S.check_bigtiff(ok)
    with pytest.raises(ValueError, match="bigtiff must be None, True or False"):
        S.check_bigtiff(1)
    assert S._optional_destination(None, (3, 5, 7), np.dtype(np.float32), None, 0) is None
    with pytest.raises(ValueError, match="bigtiff applies to a .tif / .tiff destination only"):
        S._optional_destination(None, (3, 5, 7), np.dtype(np.float32), True, 0)
    out = np.empty((3, 5, 7), np.float32)
    assert S._optional_destination(out, (3, 5, 7), np.dtype(np.float32), None, 0).target is out
