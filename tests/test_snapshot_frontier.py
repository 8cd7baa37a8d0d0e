"""Snapshot.select / Snapshot.cat on host records, and the expand entry points' bindings (no GPU)."""
import numpy as np
import pytest

from sparc_gym_amd import _lib
from sparc_gym_amd.snapshot import Snapshot
from test_snapshot_format import _info, _snap


def test_select_rows_and_masks_on_the_host():
    s = _snap(37)
    r = s.numpy()
    idx = [36, 0, 0, 5]
    mask = np.arange(37) % 5 == 1
    for snap in (s, s.to("cpu")):
        for i in (idx, np.array(idx), np.array(idx, np.int32)):
            got = snap.select(i)
            assert got.is_host and np.array_equal(got.numpy(), r[idx]) and bytes(got.info) == bytes(s.info)
        assert np.array_equal(snap.select(mask).numpy(), r[mask])
        assert len(snap.select(np.zeros(37, bool))) == 0
        with pytest.raises(ValueError):
            snap.select(np.array([1.0]))
        with pytest.raises(ValueError):
            snap.select(mask[:-1])
        with pytest.raises(ValueError):
            snap.select(np.zeros((2, 2), np.int64))
    got = s.select([3])
    got.records[:] = 0                       # a copy: the source keeps its rows
    assert np.array_equal(s.numpy(), r)


def test_cat_checks_the_headers():
    a, b = _snap(5, seed=1), _snap(9, seed=2)
    c = Snapshot.cat([a, b, a.to("cpu")])
    assert c.is_host and len(c) == 19
    assert np.array_equal(c.numpy(), np.concatenate([a.numpy(), b.numpy(), a.numpy()]))
    assert np.array_equal(Snapshot.cat([b]).numpy(), b.numpy())
    with pytest.raises(ValueError, match="traceback"):
        Snapshot.cat([a, _snap(5, traceback=0)])
    other = _info()
    other.table_hash ^= 1
    with pytest.raises(ValueError, match="table_hash"):
        Snapshot.cat([a, Snapshot(b.numpy(), other)])
    with pytest.raises(ValueError):
        Snapshot.cat([])


def test_expand_entry_points_are_bound():
    for name in ("sparc_expand_device", "sparc_expand_host"):
        assert name in _lib.EXPORTS and len(_lib._SIGS[name][0]) == 8
