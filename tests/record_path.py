"""Decode the path of state records (TEST HELPER, CPU only).

Written from the documented record layout, not from the kernels'
headers: little-endian u32 words pos (x | y<<8 | path length<<16 | off-path depth<<24), aux, step,
puzzle; then the visited board, ``words`` u64 with point (x, y) at bit x * pitch + y; then the
direction stack, 2 * ``words`` u64, move k at bits 2 * (k % 32) of word k // 32 (0 right, 1 up,
2 left, 3 down, as the actions).  The path is the start of the record's puzzle followed by the
first ``path length - 1`` moves.

``decode`` asserts what every valid record must satisfy on its own: the path ends at (x, y), its
points are distinct and inside the lattice, and the visited board holds exactly the path's points.
The one-word kernels rebuild the stored board at every store as "open and not free, plus the
start" (the canonical stored form): for a state that began at a reset with
fresh planes that is the path's points again, start included even where the start is a gap, so
the comparison is the same at every width.  A board that was given stale bits on purpose
(``sparc_set_visited_host``) holds more than the path; ``allow_extra_visited`` then checks
containment only.  With one word every stack field at or above ``path length - 1`` must be zero;
with two or four words those fields are documented as stale and are ignored.
"""
import numpy as np

DIRS = ((1, 0), (0, -1), (-1, 0), (0, 1))   # right, up, left, down


def _host(records):
    if hasattr(records, "records"):           # a Snapshot
        records = records.records
    if hasattr(records, "detach"):
        records = records.detach().cpu().numpy()
    return np.ascontiguousarray(records, np.uint8)


def decode(records, info, proc, allow_extra_visited=False):
    """records [M, record_bytes] uint8 (numpy, a tensor or a Snapshot), ``info`` with ``words``,
    ``pitch``, ``traceback`` and ``record_bytes``, ``proc`` the processed puzzles of the table.
    Returns a list of dicts: x, y, path_len, step, puzzle, path (list of (x, y)), visited (set of
    (x, y)).  AssertionError on a record that is not consistent with itself."""
    rec = _host(records)
    W, pitch, rb = int(info.words), int(info.pitch), int(info.record_bytes)
    assert info.traceback, "only traceback records hold the path's moves"
    assert W in (1, 2, 4) and rb == (16 + 24 * W + 15) // 16 * 16
    assert rec.ndim == 2 and rec.shape[1] == rb
    out = []
    for j, row in enumerate(rec):
        pos, _aux, step, pid = (int(v) for v in row[:16].view("<u4"))
        x, y, n = pos & 0xFF, (pos >> 8) & 0xFF, (pos >> 16) & 0xFF
        board = [int(v) for v in row[16:16 + 8 * W].view("<u8")]
        stack = [int(v) for v in row[16 + 8 * W:16 + 24 * W].view("<u8")]
        assert not row[16 + 24 * W:].any(), f"record {j}: padding not zero"
        assert 0 <= pid < len(proc), f"record {j}: puzzle {pid}"
        p = proc[pid]
        X, Y = int(p["x_size"]), int(p["y_size"])
        assert n >= 1, f"record {j}: path length 0"
        path = [tuple(int(v) for v in p["start_location"])]
        for k in range(n - 1):
            d = (stack[k // 32] >> (2 * (k % 32))) & 3
            path.append((path[-1][0] + DIRS[d][0], path[-1][1] + DIRS[d][1]))
        assert path[-1] == (x, y), f"record {j}: the path ends at {path[-1]}, the agent is at {(x, y)}"
        assert all(0 <= a < X and 0 <= b < Y for a, b in path), f"record {j}: the path leaves the lattice"
        assert len(set(path)) == n, f"record {j}: the path visits a point twice"
        visited = set()
        for w, v in enumerate(board):
            while v:
                b = (v & -v).bit_length() - 1 + 64 * w
                v &= v - 1
                assert b % pitch < Y and b // pitch < X, f"record {j}: visited bit {b} outside the lattice"
                visited.add((b // pitch, b % pitch))
        if allow_extra_visited:
            assert set(path) <= visited, f"record {j}: path points missing from the board"
        else:
            assert set(path) == visited, f"record {j}: the board differs from the path's points"
        if W == 1:   # canonical: only the path's moves are set
            for k in range(n - 1, 64):
                assert (stack[k // 32] >> (2 * (k % 32))) & 3 == 0, f"record {j}: stack field {k} above the top is set"
        out.append({"x": x, "y": y, "path_len": n, "step": step, "puzzle": pid, "path": path, "visited": visited})
    return out


def encode(info, pid, path, pitch=None, stale=None, step=0, aux=0, off=0):
    """A record by hand, from the same documented layout (for the decoder's own tests): the path's
    points, optionally ``stale`` = {field index: move} written above the top of the stack."""
    W, rb = int(info.words), int(info.record_bytes)
    pitch = int(info.pitch) if pitch is None else pitch
    n = len(path)
    board, stack = [0] * W, [0] * (2 * W)
    for a, b in path:
        bit = a * pitch + b
        board[bit // 64] |= 1 << (bit % 64)
    for k in range(n - 1):
        d = DIRS.index((path[k + 1][0] - path[k][0], path[k + 1][1] - path[k][1]))
        stack[k // 32] |= d << (2 * (k % 32))
    for k, d in (stale or {}).items():
        assert k >= n - 1
        stack[k // 32] |= d << (2 * (k % 32))
    row = np.zeros(rb, np.uint8)
    x, y = path[-1]
    row[:16] = np.array([x | (y << 8) | (n << 16) | (off << 24), aux, step, pid], "<u4").view(np.uint8)
    row[16:16 + 8 * W] = np.array(board, "<u8").view(np.uint8)
    row[16 + 8 * W:16 + 24 * W] = np.array(stack, "<u8").view(np.uint8)
    return row
