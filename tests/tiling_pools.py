"""Crafted poly / ylop tilings for the exact-fit search of the rule audit.  TEST INFRASTRUCTURE ONLY.

Every record is built around one or more exact-fit problems (_polyfit_region_exact,
SPaRC_Gym.py:736-853) whose area check passes, so that the search itself decides the answer: a
fitting tiling and a near-miss twin with the same areas (one piece replaced by another of equal
area) that must be refused.  Regions are the whole board, or are cut out by full walls of gap
points, or by the puzzle's first solution path (walking it then audits every step on the way).
Instances sit on cell centres of their own region, one per cell, in list order: the reference
tries polys in that order, so the order decides how much the search backtracks.

Categories (the letter is part of the record id, ``tile-<letter>-<name>``):
  a  tilings that backtrack: the first shape tried at the first negative cell is wrong
  b  shapes whose anchor is not their left-most column (negative dy): S / Z, T, plus
  c  repeated shapes (counts 2-5), and two polyshape names with identical arrays
  d  ylops that matter: inside the region, outside it, identical, different, larger than the grid
  e  pieces exactly as wide / tall as the grid, and pieces that can be placed nowhere
  f  the cell grids the code distinguishes: 3x3, 2x5, 5x2, 1x7, 7x1, 4x4, 5x7, 7x7
  g  more than 16 distinct poly shapes on 7x7 cells: the host-only search
  h  six or more static regions with instances and different answers

Grids are written x-major: row k of a grid is cell row cx = k, its characters cy = 0, 1, ...; a
shape array is indexed [dx][dy] the same way (_get_offsets 840-855).  The choices that need a
search (instance order, which piece a twin replaces) are made here with the counting port of
the oracle below; what a case answers is recorded from the reference itself when the golden files
are made (tests/golden/make_rules_golden.py), never from this file.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import rules_ref

NODE_LIMIT = 6000          # place_polys calls of one search in a crafted case (the reference is Python)
HOST_NODE_LIMIT = 8000    # ... of the host-only puzzle, whose search has to be a real one
HOST_SHAPE_LIMIT = 12000  # ... and of the same search with the shapes tried in exact_fit's order
# The middle GPU node cap of tests/test_gpu_exact_fit.py: the median node count (the smallest cap at
# which exact_fit finishes) over the searches of the recorded crafted pools, as the CPU harness prints
# them (tests/test_exact_fit_host.py::test_middle_fit_cap_is_the_crafted_pools_median asserts it).
MID_FIT_CAP = 8


# ---------------------------------------------------------------- the counting oracle
class SearchTooLong(Exception):
    pass


class CountingAudit(rules_ref.RuleAudit):
    """oracle/rules_ref.py's audit with its exact-fit searches listed: `searches` gets one entry per
    search that ran (the area check passed), with the region's cells, the answer, the ylops and the
    distinct poly names.  count=True also counts the place_polys calls and the poly placements
    undone, with a copy of the oracle's _place_polys (count=False runs the oracle's own)."""

    def __init__(self, puzzle, path, agent, limit=None, count=True, by_shape=False):
        super().__init__(puzzle, path, agent)
        self.searches, self.limit, self.by_shape = [], limit, by_shape
        if not count:
            self._place_polys = lambda polys, grid: rules_ref.RuleAudit._place_polys(self, polys, grid)

    def polyfit_exact(self, region, instances):
        self._nodes = self._undone = 0
        ok, det = super().polyfit_exact(region, instances)
        polys = [i["name"] for i in instances if i["kind"] == "poly"]
        self.searches.append({"cells": tuple(sorted(region.cells)), "ok": bool(ok),
                              "ylops": sum(i["kind"] == "ylop" for i in instances), "polys": len(polys),
                              "names": len(set(polys)), "nodes": self._nodes, "undone": self._undone})
        return ok, det

    def _place_polys(self, polys, grid):
        self._nodes += 1
        if self.limit is not None and self._nodes > self.limit:
            raise SearchTooLong()
        if np.any(grid > 0):
            return False
        if not polys:
            return not np.any(grid < 0)
        negs = np.argwhere(grid < 0)
        if negs.size == 0:
            return True
        ax, ay = (int(v) for v in negs[np.lexsort((negs[:, 1], negs[:, 0]))][0])
        if self.by_shape:     # exact_fit's order: the distinct shapes as the whole list first showed them
            if self._nodes == 1:
                self._first = {}
                for poly in polys:
                    self._first.setdefault(_key(poly["array"]), len(self._first))
            polys = sorted(polys, key=lambda poly: self._first[_key(poly["array"])])
        tried = set()
        for i, poly in enumerate(polys):
            if poly["name"] in tried:
                continue
            tried.add(poly["name"])
            offs = rules_ref._offsets(poly["array"])
            if not rules_ref._try_place(grid, offs, ax, ay, +1):
                continue
            if self._place_polys(polys[:i] + polys[i + 1:], grid):
                return True
            rules_ref._unplace(grid, offs, ax, ay, +1)
            self._undone += 1
        return False


def count_searches(puzzle, path, agent, limit=None, count=True, by_shape=False):
    a = CountingAudit(puzzle, path, agent, limit, count, by_shape)
    a.validate()
    return a.searches


# ---------------------------------------------------------------- shapes
def shape_of(cells):
    """0/1 array [dx][dy] of a set of (cx, cy) cells, in its bounding box."""
    xs, ys = [c[0] for c in cells], [c[1] for c in cells]
    arr = [[0] * (max(ys) - min(ys) + 1) for _ in range(max(xs) - min(xs) + 1)]
    for x, y in cells:
        arr[x - min(xs)][y - min(ys)] = 1
    return arr


def tiles(*rows):
    """The pieces of a label grid ('.' is no piece) as shape arrays, in order of their first cell."""
    cells = {}
    for x, row in enumerate(rows):
        for y, ch in enumerate(row):
            if ch != ".":
                cells.setdefault(ch, []).append((x, y))
    return [shape_of(c) for c in cells.values()]


def bar_x(n):
    return [[1]] * n


def bar_y(n):
    return [[1] * n]


def block(a, b):
    return [[1] * b for _ in range(a)]


def _key(arr):
    a = np.array(arr)
    xs, ys = np.where(a == 1)
    return tuple(sorted(zip((xs - xs.min()).tolist(), (ys - ys.min()).tolist())))


def variants(arr):
    """The other shapes of the same area a twin may put in a piece's place: its rotations and
    mirror images, then a bar either way."""
    a = np.array(arr)
    out, seen = [], {_key(arr)}
    cands = [np.rot90(a, k) for k in (1, 2, 3)] + [np.rot90(a.T, k) for k in (0, 1, 2, 3)]
    n = int(a.sum())
    cands += [np.array(bar_x(n)), np.array(bar_y(n))]
    for c in cands:
        if _key(c) not in seen:
            seen.add(_key(c))
            out.append(c.tolist())
    return out


# ---------------------------------------------------------------- records
def _segments(way):
    pts = [tuple(way[0])]
    for bx, by in way[1:]:
        while pts[-1] != (bx, by):
            ax, ay = pts[-1]
            pts.append((ax + (bx > ax) - (bx < ax), ay + (by > ay) - (by < ay)))
    return pts


def record(name, w, h, parts, regions=None, way=((0, 0), (0, 2))):
    """One record in the dataset's schema.  w x h cells (cx < w, cy < h).  regions: label grid
    (default: one region '0').  parts: {label: (polys, ylops)}, each a list of (shape array, name or
    None); the instances go on the region's cells in x-major order, polys first.  way: corner
    points of the first solution path; region borders that are not on it become gap points."""
    from sparc_gym_amd.synthetic import _dump
    X, Y = 2 * w + 1, 2 * h + 1
    regions = list(regions) if regions else ["0" * h] * w
    assert len(regions) == w and all(len(r) == h for r in regions), name
    path = _segments(way)
    assert len(set(path)) == len(path) and all(0 <= x < X and 0 <= y < Y and not (x % 2 and y % 2) for x, y in path)
    assert path[-1][0] in (0, X - 1) or path[-1][1] in (0, Y - 1)
    label = lambda cx, cy: regions[cx][cy] if 0 <= cx < w and 0 <= cy < h else None   # noqa: E731
    gaps = []
    for x in range(X):
        for y in range(Y):
            if x % 2 and y % 2:
                continue
            around = {label((x + dx - 1) // 2, (y + dy - 1) // 2) for dx in (-1, 0, 1) for dy in (-1, 0, 1)
                      if (x + dx) % 2 and (y + dy) % 2} - {None}
            if len(around) > 1 and (x, y) not in path:
                gaps.append((x, y))
    cells, shapes, names = [], {}, {}
    next_name = [1000 + 37 * (sum(map(ord, name)) % 97)]

    def name_of(arr, given):
        k = (given, _key(arr) if given is None else None)
        if k not in names:
            names[k] = next_name[0]
            next_name[0] += 1
            shapes[str(names[k])] = [list(map(int, r)) for r in arr]
        assert shapes[str(names[k])] == [list(map(int, r)) for r in arr], (name, given)
        return names[k]

    for lab, (polys, ylops) in parts.items():
        spots = [(2 * cx + 1, 2 * cy + 1) for cx in range(w) for cy in range(h) if regions[cx][cy] == lab]
        inst = [("poly", p) for p in polys] + [("ylop", y) for y in ylops]
        assert len(inst) <= len(spots), (name, lab, len(inst), len(spots))
        for (x, y), (kind, (arr, given)) in zip(spots, inst):
            cells.append({"position": {"x": x, "y": y},
                          "properties": {"type": kind, "color": "red", "polyshape": name_of(arr, given)}})
    assert cells and cells[0]["properties"]["type"] == "poly", name     # a 'poly' plane, a symbol cell first
    cells += [{"position": {"x": x, "y": y}, "properties": {"gap": True}} for x, y in gaps]
    grid = [["+" if not (x % 2 and y % 2) else "." for x in range(X)] for y in range(Y)]
    for x, y in gaps:
        grid[y][x] = " "
    grid[path[0][1]][path[0][0]] = "S"
    grid[path[-1][1]][path[-1][0]] = "E"
    text = {"puzzle": {"start": {"x": path[0][0], "y": path[0][1]}, "end": {"x": path[-1][0], "y": path[-1][1]},
                       "cells": cells}}
    return {"id": name, "difficulty_level": 3, "grid_size": {"width": w, "height": h}, "solution_count": 1,
            "solutions": [{"path": [{"x": x, "y": y} for x, y in path]}],
            "polyshapes": _dump(shapes), "text_visualization": _dump(text), "puzzle_array": grid}


def final_searches(rec, limit, by_shape=False):
    """The counted searches of a record's state at the end of its first solution."""
    from sparc_gym_amd.puzzles import process_puzzles
    p = process_puzzles([rec])[0]
    path = p["solution_paths"][0]
    return count_searches(p, path, path[-1], limit, by_shape=by_shape)


# ---------------------------------------------------------------- cases
class Case:
    """One designed exact-fit problem: region `lab` of a w x h board with `polys` and `ylops`
    (lists of (array, name)); other: parts of the other regions."""

    def __init__(self, cat, name, w, h, polys, ylops=(), regions=None, lab="0", way=((0, 0), (0, 2)), other=None,
                 limit=NODE_LIMIT):
        named = lambda v: [s if isinstance(s, tuple) else (s, None) for s in v]   # noqa: E731
        self.cat, self.name, self.w, self.h = cat, name, w, h
        self.polys, self.ylops = named(polys), named(ylops)
        self.regions, self.lab, self.way, self.other, self.limit = regions, lab, way, other or {}, limit

    def rec(self, polys=None, ylops=None, tag=""):
        parts = {self.lab: (self.polys if polys is None else polys, self.ylops if ylops is None else ylops)}
        parts.update(self.other)
        return record(f"tile-{self.cat}-{self.name}{tag}", self.w, self.h, parts, self.regions, self.way)

    def mine(self, rec, by_shape=False):
        """The counted search of this case's own region at the end of the solution (None: too long)."""
        cells = {(2 * cx + 1, 2 * cy + 1) for cx in range(self.w) for cy in range(self.h)
                 if (self.regions[cx][cy] if self.regions else "0") == self.lab}
        try:
            hits = [s for s in final_searches(rec, HOST_SHAPE_LIMIT if by_shape else self.limit, by_shape)
                    if set(s["cells"]) == cells]
        except SearchTooLong:
            return None
        assert len(hits) == 1, (self.name, "the designed region's area check must pass")
        return hits[0]

    def fitting(self, need_undo=False, min_nodes=0, swaps=False):
        """The fitting record: the given instance order, or (need_undo) the first of a fixed list
        of poly orders whose search undoes a placement before it succeeds.  swaps (the host-only
        puzzle, where shapes repeat): the order must also be short with the shapes tried in
        exact_fit's order, which is another where a shape's instances are apart in the list."""
        rng = np.random.default_rng(sum(map(ord, self.name)))
        for k in range(200):
            polys = self.polys if k == 0 else [self.polys[i] for i in rng.permutation(len(self.polys))]
            if swaps and k:      # a few neighbours exchanged: a full shuffle of so many shapes never ends
                polys = list(self.polys)
                for i in rng.integers(len(polys) - 1, size=3 + k // 5):
                    polys[i], polys[i + 1] = polys[i + 1], polys[i]
            rec = self.rec(polys)
            s = self.mine(rec)
            if s is None:
                continue
            assert s["ok"], (self.name, "the designed tiling must fit")
            if (not need_undo or s["undone"] > 0) and s["nodes"] >= min_nodes:
                if swaps and self.mine(rec, by_shape=True) is None:     # short for the reference, long for exact_fit
                    continue
                self.polys = polys
                return rec
        raise AssertionError((self.name, "no instance order backtracks"))

    def twin(self):
        """The near-miss twin: the first piece (last to first) and replacement shape of equal area
        for which the search, bounded, says no."""
        for kind in ("polys", "ylops"):
            own = getattr(self, kind)
            for i in reversed(range(len(own))):
                for alt in variants(own[i][0]):
                    swapped = own[:i] + [(alt, None)] + own[i + 1:]
                    rec = self.rec(**{kind: swapped}, tag="-twin")
                    s = self.mine(rec)
                    if s is not None and not s["ok"]:
                        return rec
        raise AssertionError((self.name, "no twin"))


def random_tiling(w, h, seed, sizes=(3, 4, 5), mask=None):
    """A label grid: connected pieces grown from the first free cell (x-major) to a drawn size, over
    the cells whose mask character is '0' (default: all)."""
    rng = np.random.default_rng(seed)
    grid = [[None if mask is None or mask[x][y] == "0" else "." for y in range(h)] for x in range(w)]
    k = 0
    for x in range(w):
        for y in range(h):
            if grid[x][y] is not None:
                continue
            piece, want = [(x, y)], int(sizes[int(rng.integers(len(sizes)))])
            grid[x][y] = chr(65 + k)
            while len(piece) < want:
                nb = sorted({(a + da, b + db) for a, b in piece for da, db in ((0, 1), (0, -1), (1, 0), (-1, 0))
                             if 0 <= a + da < w and 0 <= b + db < h and grid[a + da][b + db] is None})
                if not nb:
                    break
                c = nb[int(rng.integers(len(nb)))]
                grid[c[0]][c[1]] = chr(65 + k)
                piece.append(c)
            k += 1
    return ["".join(row) for row in grid]


def _random_pair(out, cat, name, w, h, sizes, need_undo=False, regions=None, extra=None, **kw):
    """_pair over a random tiling: the first seed whose fitting order and twin are both found within
    the node limit.  extra: (polys, ylops) added to the tiling's pieces."""
    for seed in range(1, 60):
        polys = tiles(*random_tiling(w, h, seed, sizes, regions))
        case = Case(cat, name, w, h, polys + (extra[0] if extra else []), extra[1] if extra else (), regions=regions, **kw)
        try:
            fit = case.fitting(need_undo)
            twin = case.twin()
        except AssertionError:
            continue
        out += [fit, twin]
        return
    raise AssertionError((name, "no seed"))


def scattered_tiling(w, h, seed, want_shapes):
    """A tiling of w x h cells (w * h odd) by pieces of two cells that need not touch, and one of
    three, every piece a shape of its own: the reference tries the names of the polys still left in
    list order and exact_fit the distinct shapes in the order they were first seen, and with no
    shape used twice the two orders are one, so the two searches visit the same nodes (with five
    shapes used twice, an order that cost the reference 5,129 calls cost exact_fit 3.5e8 nodes, for
    the same answer).  The first piece is the two far corners; in every
    other piece the later cells lie below and to the left of the first (negative dy), so none of
    them can be anchored in cell column 0: with the corner piece mirrored (the twin) the first
    negative cell can never be covered.  Shape arrays, in order of their first cell."""
    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4000))
    for attempt in range(50):
        rng = np.random.default_rng(seed * 10000 + attempt)
        cells = {(x, y) for x in range(w) for y in range(h)} - {(0, 0), (w - 1, h - 1)}
        odd = (int(rng.integers(2, w - 1)), int(rng.integers(1, h - 2)))      # joins a piece above it
        free = cells - {odd}
        ok = lambda a, b: (a[0] < b[0] and a[1] > b[1]) or (b[0] < a[0] and b[1] > a[1])   # noqa: E731
        pairs, used, budget = [], set(), [20000]

        def solve():
            if not free:
                return True
            budget[0] -= 1
            if budget[0] < 0:
                return False
            opts = {c: [d for d in free if ok(c, d)] for c in free}
            c = min(sorted(free), key=lambda v: len(opts[v]))
            cand = [opts[c][int(i)] for i in rng.permutation(len(opts[c]))]
            off = lambda d: (abs(c[0] - d[0]), -abs(c[1] - d[1]))   # noqa: E731
            cand.sort(key=lambda d: off(d) in used)                 # shapes not used yet first
            for d in cand:
                free.difference_update((c, d))
                pairs.append(sorted((c, d)))
                fresh = off(d) not in used
                used.add(off(d))
                if solve():
                    return True
                if fresh:
                    used.discard(off(d))
                pairs.pop()
                free.update((c, d))
            return False

        if not solve():
            continue
        host = [p for p in pairs if p[0][0] < odd[0] and p[0][1] > odd[1]]
        if not host:
            continue
        host[int(rng.integers(len(host)))].append(odd)
        pieces = sorted([[(0, 0), (w - 1, h - 1)]] + pairs, key=min)
        shapes = [shape_of(p) for p in pieces]
        if len({_key(v) for v in shapes}) >= want_shapes:
            return shapes
    raise AssertionError("no scattered tiling")


def _pair(case, out, need_undo=False, min_nodes=0):
    out.append(case.fitting(need_undo, min_nodes))
    out.append(case.twin())


STRIP = ((0, 0), (0, 14))   # along the x = 0 border of a 15 x 15 lattice: no region changes


@functools.lru_cache(maxsize=None)
def pools():
    """{pool name: records}: `tilings` (7x7 lattices and smaller: one word, pitch 8), `tilings2w`
    (up to 11x11: two words), `tilings4w` (up to 15x15: four words).  Deterministic.  Only
    tests/golden/make_rules_golden.py calls it (the choices of order and twin run a few minutes of
    counted searches); the tests read what it recorded."""
    one, two, four = [], [], []
    sq3 = block(3, 3)
    # ---- a: backtracking tilings
    _pair(Case("a", "tromino3x3", 3, 3, tiles("AAB", "ACB", "CCB")), one, need_undo=True)
    _pair(Case("a", "tromino3x3b", 3, 3, tiles("ABB", "AAB", "CCC")), one, need_undo=True)
    _pair(Case("a", "tetromino4x4", 4, 4, tiles("AAAB", "ACBB", "CCDB", "CDDD")), two, need_undo=True)
    _pair(Case("a", "mixed2x5", 2, 5, tiles("AABBB", "ACCCB")), two, need_undo=True)
    _pair(Case("a", "lshape5x5", 5, 5, tiles("AAB..", "ABB..", "CCDDD", "CEEDF", "CCEFF"),
               regions=["000..", "000..", "00000", "00000", "00000"]), two, need_undo=True)
    _random_pair(four, "a", "random5x7", 5, 7, (4, 5), need_undo=True)
    _random_pair(four, "a", "ushape7x7", 7, 7, (4, 5), need_undo=True, regions=["000.000", "000.000", "000.000", "000.000", "0000000", "0000000", "0000000"])
    # ---- b: anchors right of the shape's left-most column, at both edges of the grid
    _pair(Case("b", "plus3x3", 3, 3, tiles("APB", "PPP", "CPD")), one)
    _pair(Case("b", "tee3x3", 3, 3, tiles("ATB", "TTT", "CCC")), one)
    _pair(Case("b", "ess3x3", 3, 3, tiles("ASS", "SSB", "CCC")), one)
    _pair(Case("b", "zed_left3x3", 3, 3, tiles("AZB", "ZZB", "ZCC")), one)
    _pair(Case("b", "zed_right3x3", 3, 3, tiles("AAZ", "BZZ", "BZC")), one)
    _pair(Case("b", "plus_edges4x4", 4, 4, tiles("APBB", "PPPB", "CPQD", "CQQQ")), two)
    _pair(Case("b", "edges7x7", 7, 7, tiles("APBBBQC", "PPPDQQQ", "APDDDQC"), regions=["0000000"] * 3 + ["1111111"] * 4,
               way=STRIP), four)
    # ---- c: repeated shapes; two names with one array
    _pair(Case("c", "dominoes3x3", 3, 3, tiles("AAB", "CCB", "DDE")), one)
    dom = bar_y(2)
    _pair(Case("c", "two_names3x3", 3, 3, [(dom, "n1"), (dom, "n2"), (dom, "n1"), (bar_x(3), None)]), one)
    _pair(Case("c", "counts3x3", 3, 3, tiles("ABC", "ABC", "DDD")), one)
    _pair(Case("c", "bars4x4", 4, 4, tiles("AAAB", "CCCB", "DDDB", "EEEB")), two)
    _pair(Case("c", "dominoes5x2", 5, 2, tiles("AA", "BB", "CD", "CD", "EE")), two)
    _pair(Case("c", "ells4x4", 4, 4, tiles("AAAB", "ABBB", "CCCD", "CDDD")), two)
    _pair(Case("c", "fives5x7", 5, 7, tiles("AAAAABB", "CCCCCBB", "DDDDDBE", "FFFFFEE", "GGGGGEE")), four)
    # ---- d: ylops that matter
    base = tiles("AAB", "ACB", "CCB")
    _pair(Case("d", "inside3x3", 3, 3, base + [dom], [dom]), one)
    _pair(Case("d", "outside3x3", 3, 3, [sq3], [bar_x(3)], regions=["001", "001", "001"], way=((0, 4), (6, 4))), one)
    _pair(Case("d", "stacked3x3", 3, 3, [sq3, sq3, sq3], [sq3, sq3]), one)
    _pair(Case("d", "identical2_3x3", 3, 3, [sq3, dom, dom], [dom, dom]), one)
    _pair(Case("d", "identical3_3x3", 3, 3, [sq3, dom, dom, dom], [dom, dom, dom]), one)
    _pair(Case("d", "different3x3", 3, 3, [sq3, tiles("A.", "AA")[0], [[1]]], [dom, bar_x(2)]), one)
    one.append(Case("d", "giant_ylop3x3", 3, 3, [sq3, block(2, 2)], [bar_y(4)]).rec(tag="-no"))
    one.append(Case("d", "giant_ylop_x3x3", 3, 3, [sq3, block(2, 2)], [bar_x(4)]).rec(tag="-no"))
    _pair(Case("d", "outside4x4", 4, 4, [block(4, 4)], [block(2, 2)], regions=["0000", "0000", "0011", "0011"]), two)
    ell = tiles("AA", ".A")[0]
    _random_pair(four, "d", "inside5x7", 5, 7, (4, 5), extra=([ell], [ell]))
    # ---- e: as wide or as tall as the grid; wider or taller
    e32 = Case("e", "tall3x2", 3, 2, [bar_x(3), bar_x(3)])
    one.append(e32.fitting())
    one.append(Case("e", "too_tall2x3", 2, 3, [bar_x(3), bar_x(3)]).rec(tag="-no"))
    e23 = Case("e", "wide2x3", 2, 3, [bar_y(3), bar_y(3)])
    one.append(e23.fitting())
    one.append(Case("e", "too_wide3x2", 3, 2, [bar_y(3), bar_y(3)]).rec(tag="-no"))
    one.append(Case("e", "square3x3", 3, 3, [sq3]).fitting())
    one.append(Case("e", "bar9_y3x3", 3, 3, [bar_y(9)]).rec(tag="-no"))     # dy up to 8: bits of three rows
    one.append(Case("e", "bar9_x3x3", 3, 3, [bar_x(9)]).rec(tag="-no"))
    _pair(Case("e", "bars7x7", 7, 7, [bar_y(7)] * 4 + [bar_x(3)] * 7), four)
    rows = ["0000000", "0001111", "1111111"] + ["2222222"] * 4
    four.append(Case("e", "bar10_x7x7", 7, 7, [bar_x(10)], regions=rows, way=STRIP,
                     other={"1": ([(bar_x(11), None)], [])}).rec(tag="-no"))   # cell 63, and past it
    four.append(Case("e", "bar8_y7x7", 7, 7, [bar_y(8), [[1]], [[1]]], regions=rows, way=STRIP,
                     other={"1": ([(block(2, 7), None)], [])}).rec(tag="-no"))
    # ---- f: cell grids
    _pair(Case("f", "grid3x3", 3, 3, tiles("AAB", "CBB", "CCD")), one)
    _pair(Case("f", "grid2x5", 2, 5, tiles("AAABB", "CCCCB")), two)
    _pair(Case("f", "grid5x2", 5, 2, tiles("AB", "AB", "AC", "DC", "DD")), two)
    _random_pair(two, "f", "grid4x4", 4, 4, (3, 4))
    _pair(Case("f", "grid1x7", 1, 7, [bar_y(3), bar_y(4)]), four)
    _pair(Case("f", "grid7x1", 7, 1, [bar_x(4), bar_x(3)], way=((0, 0), (2, 0))), four)
    _random_pair(four, "f", "grid5x7", 5, 7, (4, 5))
    _random_pair(four, "f", "grid7x7", 7, 7, (5,))
    # ---- g: the host-only search
    g = Case("g", "host7x7", 7, 7, scattered_tiling(7, 7, 1, 20), limit=HOST_NODE_LIMIT)
    four.append(g.fitting(need_undo=True, min_nodes=300, swaps=True))
    corner = [[0] * 7 for _ in range(7)]
    corner[0][6] = corner[6][0] = 1
    assert _key(g.polys[[_key(p[0]) for p in g.polys].index(_key(shape_of([(0, 0), (6, 6)])))][0])
    twin = [(corner, None) if _key(p[0]) == _key(shape_of([(0, 0), (6, 6)])) else p for p in g.polys]
    four.append(g.rec(twin, tag="-twin"))
    # ---- h: six and more static regions with different answers
    one.append(record("tile-h-six3x3", 3, 3, {"0": ([(dom, None)], []), "1": ([([[1]], None)], []),
                                               "2": ([(bar_x(2), None)], []), "3": ([(dom, None)], []),
                                               "4": ([(bar_x(2), None)], []), "5": ([([[1]], None)], [])},
                      regions=["001", "223", "445"], way=((0, 0), (0, 2))))
    one.append(record("tile-h-six3x3b", 3, 3, {"0": ([(bar_x(2), None)], []), "1": ([([[1]], None)], []),
                                                "2": ([(dom, None)], []), "3": ([([[1]], None)], []),
                                                "4": ([(bar_x(2), None)], []), "5": ([(dom, None)], [])},
                      regions=["012", "012", "345"], way=((0, 0), (2, 0))))
    n = lambda v: [(s, None) for s in v]   # noqa: E731
    four.append(record("tile-h-strips7x7", 7, 7, {
        "0": (n([bar_y(7)]), []), "1": (n([bar_x(7)]), []), "2": (n([bar_y(3), bar_y(4)]), []),
        "3": (n([bar_y(3), block(2, 2)]), []), "4": (n([bar_y(7), dom]), n([dom])),
        "5": (n([bar_y(4), bar_y(4)]), n([[[1]]])), "6": (n([bar_y(6), bar_x(2)]), n([[[1]]]))},
        regions=[str(k) * 7 for k in range(7)], way=STRIP))
    return {"tilings": one, "tilings2w": two, "tilings4w": four}


def category(rec_id):
    """The category letter of a crafted record id."""
    assert rec_id.startswith("tile-"), rec_id
    return rec_id.split("-")[1]


def coverage(golden_pools):
    """{category: counts} over golden pools (loaded dicts): distinct searches (puzzle, region cells)
    whose area check passed, by answer, with the most ylops and distinct names of one search, the
    fitting searches that undid a poly placement, the cell grids (CX, CY) searched and whether a
    search on 7x7 cells holds cell (6, 6).  Reference-side code only."""
    from rules_io import ref_puzzle, snapshots
    out = {}
    for g in golden_pools:
        puzzles = [ref_puzzle(p) for p in g["processed"]]
        seen = set()
        for _, pi, _, s in snapshots(g):
            key = (pi, tuple(map(tuple, s["path"])))
            if key in seen:
                continue
            seen.add(key)
            for srch in count_searches(puzzles[pi], s["path"], s["agent"]):
                k2 = (pi, srch["cells"])
                if k2 in seen:
                    continue
                seen.add(k2)
                c = out.setdefault(category(g["records"][pi]["id"]),
                                   {"fit": 0, "nofit": 0, "ylops": 0, "names": 0, "fit_undone": 0, "ylop_searches": 0,
                                    "nodes": 0, "cells": 0, "grids": set(), "last_cell": False})
                c["fit" if srch["ok"] else "nofit"] += 1
                c["ylops"] = max(c["ylops"], srch["ylops"])
                c["names"] = max(c["names"], srch["names"])
                c["ylop_searches"] += srch["ylops"] > 0
                c["fit_undone"] += srch["ok"] and srch["undone"] > 0
                c["nodes"] = max(c["nodes"], srch["nodes"])
                c["cells"] = max(c["cells"], len(srch["cells"]))
                grid = ((puzzles[pi]["x_size"] - 1) // 2, (puzzles[pi]["y_size"] - 1) // 2)   # cells (CX, CY)
                c["grids"].add(grid)
                c["last_cell"] |= grid == (7, 7) and (13, 13) in srch["cells"]          # cell row 6, column 6: bit 48
    return out
