"""Target reachability of a position, from the definition alone (numpy, CPU): a plain breadth-first
search over a processed puzzle's ``gaps`` array and a visited plane.  The yardstick of
``SPaRCVecEnv.reach`` / ``sparc_reach_records_device``; tests/test_reach_ref.py pins it on hand-made
boards.

For a puzzle, an agent at (x, y) and a visited plane V:
  F            the lattice points that are no gap and not in V
  C, D         the 4-connected component of F that holds the target and the breadth-first distance
               to the target inside it (C empty when the target is not in F)
  action_dist  1 + D(n_a) when the neighbour n_a in direction a lies in the lattice and in C, else 255
  live         bit a set iff action_dist[a] != 255
  dist         0 on the target, else min(action_dist), 255 when there is none
  size         |C|
  plane        D on C, 255 elsewhere, [x_dim, y_dim]
The action order is the step's: 0 (+1, 0), 1 (0, -1), 2 (-1, 0), 3 (0, +1)."""
from collections import deque

import numpy as np

NONE = 255
DIRS = ((1, 0), (0, -1), (-1, 0), (0, 1))


def reach_one(puzzle, x, y, visited, x_dim=None, y_dim=None):
    """(dist, action_dist [4], live, size, plane [x_dim, y_dim]) of one position; ``visited`` is any
    array indexed [x, y] that covers the puzzle's lattice, nonzero where the path has been."""
    X, Y = int(puzzle["x_size"]), int(puzzle["y_size"])
    x_dim, y_dim = X if x_dim is None else x_dim, Y if y_dim is None else y_dim
    gaps = np.asarray(puzzle["obs_array"]["gaps"])
    tx, ty = (int(v) for v in puzzle["target_location"])
    free = lambda a, b: 0 <= a < X and 0 <= b < Y and gaps[a, b] == 0 and visited[a, b] == 0  # noqa: E731
    plane = np.full((x_dim, y_dim), NONE, np.uint8)
    D = {}
    if free(tx, ty):
        D[(tx, ty)] = 0
        todo = deque([(tx, ty)])
        while todo:
            a, b = todo.popleft()
            for dx, dy in DIRS:
                n = (a + dx, b + dy)
                if n not in D and free(*n):
                    D[n] = D[(a, b)] + 1
                    todo.append(n)
    for (a, b), d in D.items():
        plane[a, b] = d
    ad = np.full(4, NONE, np.uint8)
    for k, (dx, dy) in enumerate(DIRS):
        n = (int(x) + dx, int(y) + dy)
        if n in D:
            ad[k] = 1 + D[n]
    live = sum(1 << k for k in range(4) if ad[k] != NONE)
    dist = 0 if (int(x), int(y)) == (tx, ty) else int(ad.min())
    return dist, ad, live, len(D), plane


def reach(proc, pid, x, y, visited, x_dim, y_dim):
    """The five outputs for n positions, as uint8 arrays: ``pid``, ``x``, ``y`` [n], ``visited``
    [n, >= x_dim, >= y_dim]."""
    n = len(pid)
    out = {"dist": np.empty(n, np.uint8), "action_dist": np.empty((n, 4), np.uint8), "live": np.empty(n, np.uint8),
           "size": np.empty(n, np.uint8), "plane": np.empty((n, x_dim, y_dim), np.uint8)}
    for i in range(n):
        d, ad, lv, sz, pl = reach_one(proc[int(pid[i])], x[i], y[i], visited[i], x_dim, y_dim)
        out["dist"][i], out["action_dist"][i], out["live"][i], out["size"][i], out["plane"][i] = d, ad, lv, sz, pl
    return out


def forward_legal(puzzle, x, y, visited):
    """The forward legal moves (_get_legal_actions without the traceback pop) as a 4-bit mask."""
    X, Y = int(puzzle["x_size"]), int(puzzle["y_size"])
    gaps = np.asarray(puzzle["obs_array"]["gaps"])
    m = 0
    for k, (dx, dy) in enumerate(DIRS):
        a, b = int(x) + dx, int(y) + dy
        if 0 <= a < X and 0 <= b < Y and gaps[a, b] == 0 and visited[a, b] == 0:
            m |= 1 << k
    return m
