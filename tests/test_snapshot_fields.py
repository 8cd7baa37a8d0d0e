"""Snapshot.fields() on records built by hand from the documented layout: bytes
0-3 pos = x | y<<8 | path length<<16 | off-path depth<<24, 4-7 aux, 8-11 current_step, 12-15
puzzle index, then the visited board and (traceback) the direction stack.  No GPU."""
import ctypes

import numpy as np
import pytest

from sparc_gym_amd import _lib
from sparc_gym_amd.snapshot import Snapshot, record_bytes


def _info(words, tb):
    return _lib.SparcSnapshotInfo(_lib.SNAPSHOT_MAGIC, 2, words, 8 if words == 1 else 12, int(tb), 2000,
                                  record_bytes(words, tb), 0, 0x1234)


def _records(words, tb, M=37, seed=0):
    rng = np.random.default_rng(seed + 10 * words + int(tb))
    want = {"x": rng.integers(0, 15, M), "y": rng.integers(0, 15, M), "path_len": rng.integers(1, 226, M),
            "step": rng.integers(0, 2**31, M), "puzzle_index": rng.integers(0, 2**32, M)}
    want["step"][0], want["puzzle_index"][0] = 2**32 - 1, 2**32 - 1          # the fields are unsigned
    off = rng.integers(0, 256, M)
    w = np.zeros((M, record_bytes(words, tb) // 4), "<u4")
    w[:, 0] = want["x"] | (want["y"] << 8) | (want["path_len"] << 16) | (off << 24)
    w[:, 1] = rng.integers(0, 2**20, M)                                       # aux: not a field
    w[:, 2] = want["step"]
    w[:, 3] = want["puzzle_index"]
    w[:, 4:] = rng.integers(0, 2**32, (M, w.shape[1] - 4))                    # boards and stack: noise to the decoder
    return np.ascontiguousarray(w).view(np.uint8).reshape(M, -1), want


@pytest.mark.parametrize("tb", [False, True])
@pytest.mark.parametrize("words", [1, 2])
def test_fields_decode_the_documented_layout(words, tb):
    rec, want = _records(words, tb)
    assert rec.shape[1] == {(1, False): 32, (1, True): 48, (2, False): 32, (2, True): 64}[(words, tb)]
    keep = rec.copy()
    snap = Snapshot(rec, _info(words, tb))
    got = snap.fields()
    assert sorted(got) == ["path_len", "puzzle_index", "step", "x", "y"]
    for k, v in want.items():
        assert isinstance(got[k], np.ndarray) and got[k].shape == (len(rec),)
        assert np.array_equal(got[k], v.astype(np.int64)), k
    assert np.array_equal(snap.records, keep)                                 # read-only
    torch = pytest.importorskip("torch")
    t = Snapshot(torch.from_numpy(rec.copy()), _info(words, tb)).fields()     # the tensor path, on the CPU
    for k, v in want.items():
        assert isinstance(t[k], torch.Tensor) and np.array_equal(t[k].numpy(), v.astype(np.int64)), k
    sub = snap.select([5, 0, 5]).fields()
    assert np.array_equal(sub["step"], want["step"][[5, 0, 5]])


def test_solver_is_exported():
    pytest.importorskip("torch")
    from sparc_gym_amd import search
    assert callable(search.solve_by_rules) and callable(search.expand_frontier) and callable(search.enumerate_paths)
    assert search.RULE_ALL == 1 << 8 and ctypes.sizeof(_lib.SparcSnapshotInfo) == 40
    assert {"sparc_rules_records_device", "sparc_rules_records_host"} <= set(_lib.EXPORTS)
