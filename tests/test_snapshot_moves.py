"""Snapshot.moves(): the action lists of traceback records, against the test helper's own reading of
the documented layout (tests/record_path.py encode / decode; move k at bits 2 (k % 32) of stack
word k // 32, the first path length - 1 moves).  Records built by hand, no GPU."""
import numpy as np
import pytest

from long_pools import column_snake, walk
from record_path import DIRS, decode, encode
from sparc_gym_amd import _lib
from sparc_gym_amd.snapshot import Snapshot, record_bytes

# words, pitch, lattice side: 7 x 7 padded, 9 x 9, 15 x 15
SHAPES = {1: (8, 7), 2: (9, 9), 4: (15, 15)}
LENGTHS = (1, 2, 3, 32, 33, 34, 49, 64, 65, 66, 81, 128, 129, 225)


def _info(words, tb=True):
    return _lib.SparcSnapshotInfo(_lib.SNAPSHOT_MAGIC, 2, words, SHAPES[words][0], int(tb), 2000,
                                  record_bytes(words, tb), 0, 0x1234)


def _paths(words):
    X = SHAPES[words][1]
    full = walk((0, 0), column_snake(X, X, 0))
    assert len(full) == X * X
    return [full[:n] for n in LENGTHS if n <= len(full)]


def _actions(path):
    return [DIRS.index((b[0] - a[0], b[1] - a[1])) for a, b in zip(path[:-1], path[1:])]


@pytest.mark.parametrize("words", [1, 2, 4])
def test_moves_equal_the_encoded_paths(words):
    info = _info(words)
    paths = _paths(words)
    rec = np.stack([encode(info, 0, p, step=len(p)) for p in paths])
    snap = Snapshot(rec, info)
    keep = rec.copy()
    got = snap.moves()
    assert np.array_equal(rec, keep)                                         # read-only
    assert isinstance(got, list) and len(got) == len(paths)
    assert max(len(g) for g in got) == SHAPES[words][1] ** 2 - 1            # the longest path the lattice holds
    for p, g in zip(paths, got):
        assert isinstance(g, list) and all(type(a) is int for a in g)
        assert g == _actions(p)
    proc = [{"x_size": SHAPES[words][1], "y_size": SHAPES[words][1], "start_location": [0, 0]}]
    for d, g in zip(decode(rec, info, proc), got):                           # and the helper's decoder agrees
        assert _actions(d["path"]) == g


@pytest.mark.parametrize("words", [2, 4])
def test_stale_fields_above_the_top_are_not_read(words):
    """With more than one word the fields at and above the top hold whatever a longer path left."""
    info = _info(words)
    paths = [p for p in _paths(words) if len(p) < SHAPES[words][1] ** 2]
    rec = []
    for p in paths:
        n = len(p)
        stale = {k: (k * 7 + 3) % 4 for k in {n - 1, n, n + 5, 31, 32, 63, 64 * words - 1} if k >= n - 1}
        rec.append(encode(info, 0, p, stale=stale))
    clean = Snapshot(np.stack([encode(info, 0, p) for p in paths]), info).moves()
    got = Snapshot(np.stack(rec), info).moves()
    assert got == clean == [_actions(p) for p in paths]
    assert any(len(g) == 0 for g in got) and any(len(g) > 32 for g in got)


def test_tensor_records_and_zeroed_records():
    torch = pytest.importorskip("torch")
    info = _info(1)
    paths = _paths(1)
    rec = np.stack([encode(info, 0, p) for p in paths] + [np.zeros(info.record_bytes, np.uint8)])
    want = [_actions(p) for p in paths] + [[]]                               # path length 0: no record
    assert Snapshot(torch.from_numpy(rec), info).moves() == want
    assert Snapshot(rec[:0], info).moves() == []


def test_records_without_traceback_hold_no_moves():
    info = _info(1, tb=False)
    snap = Snapshot(np.zeros((3, info.record_bytes), np.uint8), info)
    with pytest.raises(ValueError, match="traceback"):
        snap.moves()
