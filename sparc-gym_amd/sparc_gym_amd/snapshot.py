"""Snapshot: the state of M envs as opaque fixed-size records, with the header that says which
contexts may take them back (include/sparc_gym_amd.h, sparc_snapshot_info).

The reference has no counterpart; its user copies the ``SPaRC_Gym`` object (the per-episode
fields of ``_load_puzzle``, SPaRC_Gym.py:141-187).  ``SPaRCVecEnv.snapshot()`` returns one of
these, ``SPaRCVecEnv.restore(snap, src)`` writes record ``src[i]`` into env ``i``, and
``save`` / ``load`` keep it in a file.

File format (little endian, numpy only, no pickle)::

    offset  0  8 bytes   b"SPRCSNAP"
            8  u32       file format version (1)
           12  u32       header bytes H (40 = sizeof(sparc_snapshot_info))
           16  u64       M, the number of records
           24  H bytes   sparc_snapshot_info: magic u32, abi_version, words, pitch, traceback,
                         max_steps, record_bytes, reserved (i32 each), table_hash u64
         24+H  M * record_bytes bytes: the records
          end  u32       zlib.crc32 of the records
"""
from __future__ import annotations

import ctypes
import zlib

import numpy as np

from . import _lib

FILE_MAGIC = b"SPRCSNAP"
FILE_VERSION = 1
_HEAD = 24
INFO_FIELDS = ("words", "pitch", "traceback", "max_steps", "record_bytes", "table_hash")


def record_bytes(words, traceback):
    """Bytes of one record: pos, aux, step, puzzle (16 B), the visited board (8 * words) and,
    with traceback, the direction stack (16 * words), rounded up to a multiple of 16."""
    if words not in (1, 2, 4):
        raise ValueError("words must be 1, 2 or 4")
    return (16 + 8 * words + (16 * words if traceback else 0) + 15) // 16 * 16


def _copy_info(info):
    out = _lib.SparcSnapshotInfo()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(info), ctypes.sizeof(out))
    return out


def info_mismatch(a, b):
    """Name of the first header field in which two sparc_snapshot_info differ, or None."""
    for f in INFO_FIELDS:
        if getattr(a, f) != getattr(b, f):
            return f
    return None


class Snapshot:
    """``records``: uint8 [M, record_bytes], a torch tensor (GPU or CPU) or a numpy array;
    ``info``: the ``_lib.SparcSnapshotInfo`` of the context that wrote them."""

    def __init__(self, records, info):
        if records.ndim != 2 or records.shape[1] != info.record_bytes:
            raise ValueError(f"records must be [M, {info.record_bytes}] uint8")
        if info.magic != _lib.SNAPSHOT_MAGIC:
            raise ValueError("bad snapshot header magic")
        self.records = records
        self.info = _copy_info(info)

    def __len__(self):
        return int(self.records.shape[0])

    @property
    def is_host(self):
        return isinstance(self.records, np.ndarray) or self.records.device.type == "cpu"

    def numpy(self):
        """The records as a C-contiguous numpy array on the host (a copy if they are on the GPU)."""
        r = self.records
        if not isinstance(r, np.ndarray):
            r = r.detach().cpu().numpy()
        return np.ascontiguousarray(r, np.uint8)

    def cpu(self):
        if isinstance(self.records, np.ndarray):
            return self
        return Snapshot(self.records.cpu(), self.info)

    def to(self, device):
        import torch
        r = self.records
        if isinstance(r, np.ndarray):
            r = torch.from_numpy(np.ascontiguousarray(r, np.uint8))
        return Snapshot(r.to(device), self.info)

    def fields(self):
        """The scalar fields of every record, decoded by the documented layout (bytes 0-15: pos =
        x | y<<8 | path length<<16 | off-path depth<<24, aux, current_step, puzzle index): a dict
        of ``x``, ``y``, ``path_len``, ``step``, ``puzzle_index``, each [M] int64, as numpy arrays
        for host records and tensors on the records' device otherwise.  Read-only: new arrays,
        the records are not changed.  ``path_len`` is the number of points on the path (1 after a
        reset): a traceback pop gives a child one shorter than its parent, a forward move one
        longer."""
        r = self.records
        if isinstance(r, np.ndarray):
            w = np.ascontiguousarray(r[:, :16], np.uint8).view("<u4").astype(np.int64)   # [M, 4]
        else:
            import torch
            b = r[:, :16].to(torch.int64).reshape(len(r), 4, 4)   # little-endian bytes of the 4 words
            w = b[:, :, 0] | (b[:, :, 1] << 8) | (b[:, :, 2] << 16) | (b[:, :, 3] << 24)
        pos = w[:, 0]
        return {"x": pos & 0xFF, "y": (pos >> 8) & 0xFF, "path_len": (pos >> 16) & 0xFF, "step": w[:, 2],
                "puzzle_index": w[:, 3]}

    def moves(self):
        """The action lists of traceback records: per record the first ``path_len - 1`` moves of its
        direction stack, the path from the puzzle's start as actions (0 right, 1 up, 2 left, 3
        down).  Move k sits at bits ``2 * (k % 32)`` of stack word ``k // 32``, the stack follows the
        ``words`` u64 of the visited board; fields at and above the top (stale with more than one
        word) are not read.  A list of lists of ints, on the host (GPU records are copied); a
        zeroed record (path length 0) gives an empty list.  ValueError on records without
        traceback: they hold no moves."""
        if not self.info.traceback:
            raise ValueError("only traceback records hold the path's moves")
        rec = self.numpy()
        W = int(self.info.words)
        if len(rec) == 0:
            return []
        n = ((rec[:, :4].copy().view("<u4")[:, 0] >> 16) & 0xFF).astype(np.int64)
        stack = np.ascontiguousarray(rec[:, 16 + 8 * W:16 + 24 * W]).view("<u8")          # [M, 2W]
        k = np.arange(64 * W)
        field = ((stack[:, k // 32] >> (2 * (k % 32)).astype(np.uint64)) & np.uint64(3)).astype(np.int64)
        return [[int(a) for a in field[j, :max(int(n[j]) - 1, 0)]] for j in range(len(rec))]

    # ------------------------------------------------------------------ frontiers
    def select(self, idx):
        """A new ``Snapshot`` of rows ``idx``: a tensor, array or list of integers (any order,
        repeats allowed) or a bool mask over the records.  Stays where the records are."""
        r = self.records
        if isinstance(r, np.ndarray):
            i = idx.detach().cpu().numpy() if hasattr(idx, "detach") else np.asarray(idx)
            if i.dtype != np.bool_ and i.dtype.kind not in "iu":
                raise ValueError("idx must hold integers or be a bool mask")
            if i.ndim != 1 or (i.dtype == np.bool_ and len(i) != len(r)):
                raise ValueError("idx must be one-dimensional (a mask: one entry per record)")
            return Snapshot(np.ascontiguousarray(r[i]), self.info)
        import torch
        i = torch.as_tensor(idx, device=r.device)
        if i.dtype.is_floating_point or i.dtype.is_complex:
            raise ValueError("idx must hold integers or be a bool mask")
        if i.ndim != 1 or (i.dtype == torch.bool and len(i) != len(r)):
            raise ValueError("idx must be one-dimensional (a mask: one entry per record)")
        if i.dtype not in (torch.bool, torch.int64):
            i = i.to(torch.int64)
        return Snapshot(r[i].contiguous(), self.info)

    @classmethod
    def cat(cls, snaps):
        """The records of ``snaps`` in order, as one ``Snapshot``.  ValueError naming the field if
        their headers differ; on the GPU if the first one's records are (the others are moved)."""
        snaps = list(snaps)
        if not snaps:
            raise ValueError("nothing to concatenate")
        first = snaps[0]
        for s in snaps[1:]:
            bad = info_mismatch(first.info, s.info)
            if bad is not None:
                raise ValueError(f"snapshots do not match: {bad} differs")
        if isinstance(first.records, np.ndarray):
            return cls(np.concatenate([s.numpy() for s in snaps]), first.info)
        import torch
        dev = first.records.device
        return cls(torch.cat([s.to(dev).records for s in snaps]), first.info)

    # ------------------------------------------------------------------ file
    def save(self, path):
        rec = self.numpy()
        info = bytes(self.info)
        with open(path, "wb") as f:
            f.write(FILE_MAGIC)
            f.write(np.array([FILE_VERSION, len(info)], "<u4").tobytes())
            f.write(np.array([len(rec)], "<u8").tobytes())
            f.write(info)
            f.write(rec.tobytes())
            f.write(np.array([zlib.crc32(rec.tobytes()) & 0xFFFFFFFF], "<u4").tobytes())

    @classmethod
    def load(cls, path):
        """Read a file written by ``save``.  ValueError on a bad magic, a size that does not match
        the header, or a wrong checksum."""
        with open(path, "rb") as f:
            blob = f.read()
        H = ctypes.sizeof(_lib.SparcSnapshotInfo)
        if len(blob) < _HEAD + H + 4:
            raise ValueError("snapshot file too short")
        if blob[:8] != FILE_MAGIC:
            raise ValueError("not a snapshot file (bad magic)")
        version, hbytes = (int(v) for v in np.frombuffer(blob, "<u4", 2, 8))
        M = int(np.frombuffer(blob, "<u8", 1, 16)[0])
        if version != FILE_VERSION or hbytes != H:
            raise ValueError(f"unsupported snapshot file version {version} / header size {hbytes}")
        info = _lib.SparcSnapshotInfo.from_buffer_copy(blob[_HEAD:_HEAD + H])
        if info.magic != _lib.SNAPSHOT_MAGIC:
            raise ValueError("bad snapshot header magic")
        rb = info.record_bytes
        if rb < 16 or rb % 16 or info.words not in (1, 2, 4) or rb != record_bytes(info.words, info.traceback):
            raise ValueError(f"bad record size {rb} in the snapshot header")
        if len(blob) != _HEAD + H + M * rb + 4:
            raise ValueError(f"snapshot file size {len(blob)} does not match its header ({M} records of {rb} bytes)")
        payload = blob[_HEAD + H:_HEAD + H + M * rb]
        crc = int(np.frombuffer(blob, "<u4", 1, len(blob) - 4)[0])
        if zlib.crc32(payload) & 0xFFFFFFFF != crc:
            raise ValueError("snapshot file checksum mismatch")
        rec = np.frombuffer(payload, np.uint8).reshape(M, rb).copy()
        return cls(rec, info)
