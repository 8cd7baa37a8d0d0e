"""Lattices and scripted walks for the long-path tests (TEST HELPER, CPU only).

The 16x16 lattice is the largest the 256-bit board and the C oracle hold.  Gap-free it has 256
points, one more than the 8-bit path length can count, so the loaders refuse it; with point (0, 0)
closed and the start at (0, 1) it has 255, the maximum, and the column snake from (0, 1) still
covers every open point.  Like the gap-free pools of test_gpu_splitw_edges.py these are tables the
C ABI and pack_table accept though _process_puzzles never makes one (its lattices are odd-sized
and have gaps at the cell centres)."""
import copy

import numpy as np

from sparc_gym_amd import synthetic
from sparc_gym_amd.puzzles import process_puzzles

MOVES = ((1, 0), (0, -1), (-1, 0), (0, 1))   # right, up, left, down


def column_snake(X, Y, sy=0):
    """Actions from (0, sy) down column 0, right, up column 1, ...: through every point at or below
    (0, sy) in column 0 and every point of the other columns."""
    acts = [3] * (Y - 1 - sy)
    for x in range(1, X):
        acts.append(0)
        acts += [1 if x % 2 else 3] * (Y - 1)
    return acts


def row_snake(X, Y):
    """The transposed snake: right along the start's row, down, left along the next row, ...  From
    (0, sy) it stays in the lattice for (Y - sy) * X - 1 moves."""
    acts = []
    for y in range(Y):
        acts += [2 if y % 2 else 0] * (X - 1)
        acts.append(3)
    return acts[:-1]


def walk(start, acts):
    """The points of the path that `acts` walk from `start`."""
    path = [tuple(start)]
    for a in acts:
        path.append((path[-1][0] + MOVES[a][0], path[-1][1] + MOVES[a][1]))
    return path


def square_pool(size=16, closed=True):
    """Four size x size puzzles without gaps but, if `closed`, point (0, 0), started at (0, 1) then
    and at (0, 0) otherwise; targets at both corners of the last column; the one solution is the
    snake."""
    base = process_puzzles(synthetic.make_puzzles(4, seed=5, sizes=((7, 7),), full_properties=False))
    start = (0, 1) if closed else (0, 0)
    out = []
    for k, p in enumerate(base):
        q = copy.deepcopy(p)
        q["x_size"] = q["y_size"] = size
        gaps = np.zeros((size, size), np.int32)
        gaps[0, 0] = int(closed)
        q["obs_array"]["gaps"] = gaps
        q["start_location"] = list(start)
        q["target_location"] = [size - 1, size - 1] if k % 2 == 0 else [size - 1, 0]
        q["solution_paths"] = [[list(pt) for pt in walk(start, column_snake(size, size, start[1]))]]
        q["solution_count"] = 1
        out.append(q)
    return out
