"""The snapshot file format and the host side of the snapshot entry points (no GPU).

Snapshot.save / load keep the header (sparc_snapshot_info), the records and a crc32 of the
records; a damaged file is a ValueError, never a silently different state."""
import ctypes

import numpy as np
import pytest

from sparc_gym_amd import _lib
from sparc_gym_amd.snapshot import FILE_MAGIC, Snapshot, record_bytes

NEW = ("sparc_snapshot_info_get", "sparc_snapshot_device", "sparc_restore_device", "sparc_fork_device",
       "sparc_snapshot_host", "sparc_restore_host")


def _info(words=1, traceback=1):
    return _lib.SparcSnapshotInfo(_lib.SNAPSHOT_MAGIC, 2, words, 8, traceback, 2000,
                                  record_bytes(words, traceback), 0, 0x0123456789ABCDEF)


def _snap(m=37, words=1, traceback=1, seed=0):
    info = _info(words, traceback)
    rec = np.random.default_rng(seed).integers(0, 256, (m, info.record_bytes), dtype=np.uint8)
    return Snapshot(rec, info)


@pytest.mark.parametrize("words,traceback", [(1, 1), (2, 0), (4, 1)])
def test_save_load_round_trip(tmp_path, words, traceback):
    s = _snap(37, words, traceback)
    path = tmp_path / "s.snap"
    s.save(path)
    t = Snapshot.load(path)
    assert len(t) == 37 and t.is_host
    assert np.array_equal(t.numpy(), s.numpy())
    assert bytes(t.info) == bytes(s.info)
    assert t.info.table_hash == 0x0123456789ABCDEF and t.info.max_steps == 2000
    # through torch on the host and back
    u = t.to("cpu").cpu()
    assert np.array_equal(u.numpy(), s.numpy()) and len(u) == 37


def test_flipped_payload_byte_is_rejected(tmp_path):
    s = _snap()
    path = tmp_path / "s.snap"
    s.save(path)
    blob = bytearray(path.read_bytes())
    blob[24 + ctypes.sizeof(_lib.SparcSnapshotInfo) + 5 * s.info.record_bytes + 3] ^= 0x10
    path.write_bytes(bytes(blob))
    with pytest.raises(ValueError, match="checksum"):
        Snapshot.load(path)


def test_truncated_file_is_rejected(tmp_path):
    s = _snap()
    path = tmp_path / "s.snap"
    s.save(path)
    blob = path.read_bytes()
    for cut in (len(blob) - 1, len(blob) - s.info.record_bytes, 30, 3):
        path.write_bytes(blob[:cut])
        with pytest.raises(ValueError):
            Snapshot.load(path)
    path.write_bytes(blob + b"\0")
    with pytest.raises(ValueError):
        Snapshot.load(path)


def test_bad_magic_is_rejected(tmp_path):
    s = _snap()
    path = tmp_path / "s.snap"
    s.save(path)
    blob = bytearray(path.read_bytes())
    assert bytes(blob[:8]) == FILE_MAGIC
    bad = bytearray(blob)
    bad[0] ^= 0xFF
    path.write_bytes(bytes(bad))
    with pytest.raises(ValueError, match="magic"):
        Snapshot.load(path)
    bad = bytearray(blob)
    bad[24] ^= 0xFF          # the header struct's own magic
    path.write_bytes(bytes(bad))
    with pytest.raises(ValueError, match="magic"):
        Snapshot.load(path)


def test_bad_record_size_in_header_is_rejected(tmp_path):
    s = _snap()
    path = tmp_path / "s.snap"
    s.save(path)
    blob = bytearray(path.read_bytes())
    off = 24 + _lib.SparcSnapshotInfo.record_bytes.offset
    blob[off:off + 4] = np.array([40], "<i4").tobytes()   # the unpadded field sum: not a record size
    path.write_bytes(bytes(blob))
    with pytest.raises(ValueError, match="record size"):
        Snapshot.load(path)


@pytest.mark.parametrize("words", [1, 2, 4])
@pytest.mark.parametrize("traceback", [0, 1])
def test_record_bytes(words, traceback):
    """A record holds pos, aux, step, puzzle (4 B each), the visited board and, with traceback,
    the direction stack of 2 * words u64 words; padded to 16 B."""
    rb = record_bytes(words, traceback)
    fields = 16 + 8 * words + (16 * words if traceback else 0)
    assert rb % 16 == 0 and fields <= rb < fields + 16
    assert record_bytes(1, 1) == 48


def test_records_must_match_the_header():
    info = _info()
    with pytest.raises(ValueError):
        Snapshot(np.zeros((4, info.record_bytes + 16), np.uint8), info)
    with pytest.raises(ValueError):
        record_bytes(3, 1)


def test_new_entry_points_are_bound_and_exported():
    for name in NEW:
        assert name in _lib.EXPORTS
    lib = _lib.load()
    for name in NEW:
        assert getattr(lib, name).restype is ctypes.c_int32


def test_null_context_is_an_error_not_a_crash():
    lib = _lib.load()
    info = _info()
    buf = (ctypes.c_uint8 * 64)()
    assert lib.sparc_snapshot_info_get(None, ctypes.byref(info)) == -1
    assert lib.sparc_snapshot_device(None, None, 1, buf) == -1
    assert lib.sparc_restore_device(None, ctypes.byref(info), buf, 1, None, None, None) == -1
    assert lib.sparc_fork_device(None, None, None, None) == -1
    assert lib.sparc_snapshot_host(None, None, 1, buf) == -1
    assert lib.sparc_restore_host(None, ctypes.byref(info), buf, 1, None, None, None) == -1
    assert b"null context" in lib.sparc_last_error(None)
