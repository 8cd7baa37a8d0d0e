"""The observation of state records in numpy, from the documented record layout alone
(include/sparc_gym_amd.h: u32 words pos = x | y << 8 | len << 16 | off << 24, aux, step, pid, then
`words` u64 of the visited board, bit x * pitch + y): records -> (visited, agent, puzzle, loc), the
planes of _get_obs (SPaRC_Gym.py:956-979).  CPU helper: no import of the code under test (the
tests pack their tables with puzzles.pack_table and pass its words and pitch in)."""
import numpy as np


def record_bytes(words, traceback):
    return ((4 + 2 * words + (4 * words if traceback else 0) + 3) & ~3) * 4


def decode(records, words, pitch, x_dim, y_dim):
    """records [M, record_bytes] uint8 -> visited, agent [M, x_dim, y_dim] int32, puzzle [M] int64,
    loc [M, 2] int64.  Cell (x, y) of visited is board bit x * pitch + y when y < pitch and the bit
    is below 64 * words, else 0; agent is 1 exactly at (x, y)."""
    rec = np.ascontiguousarray(records, np.uint8)
    M = len(rec)
    head = rec[:, :16].copy().view("<u4").astype(np.int64)
    pos, pid = head[:, 0], head[:, 3]
    x, y = pos & 0xFF, (pos >> 8) & 0xFF
    board = rec[:, 16:16 + 8 * words].copy().view("<u8")           # [M, words]
    visited = np.zeros((M, x_dim, y_dim), np.int32)
    for cx in range(x_dim):
        for cy in range(min(y_dim, pitch)):
            b = cx * pitch + cy
            if b < 64 * words:
                visited[:, cx, cy] = ((board[:, b >> 6] >> np.uint64(b & 63)) & np.uint64(1)).astype(np.int32)
    agent = np.zeros((M, x_dim, y_dim), np.int32)
    agent[np.arange(M), x, y] = 1
    return visited, agent, pid, np.stack([x, y], axis=1)

