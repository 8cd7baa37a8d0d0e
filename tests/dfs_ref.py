"""A depth-first walker of the forward-move tree of a processed puzzle (TEST HELPER, CPU only), the
reference of SPaRCVecEnv.dfs / sparc_dfs_device.

Written from the reference's rules, not from the kernel: a move enters a lattice point that is no
gap and not on the path (_get_legal_actions, SPaRC_Gym.py:1024-1051, without the traceback pop),
actions are tried in the order 0, 1, 2, 3, and an entered node is a leaf when it is the target
(1192), when its step truncated (current_step >= max_steps, 1134, or no legal action at all, 1195:
on a traceback env that is a node without a forward move whose pop is illegal too, which only
happens at path length 2 on a start that is a gap), or when it has no forward move (a dead end).
Target leaves are audited by oracle/rules_ref.py.

The walk is pre-order, so "the first n nodes" is well defined: ``Walker.run(budget)`` enters at
most ``budget`` nodes, finishes the accounting of the last one and then only looks ahead: if no
node is left the walk is complete (the current path is the root's again), otherwise the current
path stays the last entered node's.  Repeated ``run`` calls continue where the last one stopped.
"""
import numpy as np

from oracle import rules_ref

DIRS = {0: (1, 0), 1: (0, -1), 2: (-1, 0), 3: (0, 1)}    # SPaRC_Gym.py:212-217
RULE_ALL, RULE_EXHAUSTED = 1 << 8, 1 << 9
COUNTERS = ("nodes", "targets", "satisfied", "listed", "both", "dead_ends", "truncated", "undecided")


def points_of(p, actions):
    """The lattice points of the path that starts at p's start and takes ``actions``."""
    path = [tuple(int(v) for v in p["start_location"])]
    for a in actions:
        path.append((path[-1][0] + DIRS[a][0], path[-1][1] + DIRS[a][1]))
    return path


class Walker:
    """The walk below the node reached by ``prefix`` (actions from the puzzle's start).
    ``root_step``: current_step of the root; ``undecided``: a predicate on a target leaf's entry
    (see ``leaves``) that makes it undecided instead of judged; ``searches``: also record whether
    the leaf's audit ran an exact-fit search (tests/tiling_pools.count_searches).

    After any ``run``: ``counts`` (dict of the eight counters so far), ``path`` (the current
    action list from the puzzle's start), ``complete``, ``first`` (the least decided satisfying
    action list so far, or None) and ``leaves``: {action tuple: dict(bits, listed, searched)} of
    the target leaves met so far, in walk order.  A root dead end is not an entered node: it shows
    in ``counts`` only, not in ``trace``."""

    _audits = {}    # (id of the puzzle dict, action tuple, searches) -> leaf entry: audits are the slow part

    def __init__(self, p, prefix=(), max_steps=2000, root_step=0, undecided=None, searches=False, trace=False):
        self.p = p
        self.X, self.Y = int(p["x_size"]), int(p["y_size"])
        self.gaps = np.asarray(p["obs_array"]["gaps"])
        self.target = tuple(int(v) for v in p["target_location"])
        self.listed = {tuple(tuple(int(c) for c in pt) for pt in sp)
                       for sp in p["solution_paths"][:p["solution_count"]]}
        self.max_steps, self.root_step = int(max_steps), int(root_step)
        self.undecided, self.searches = undecided, searches
        self.acts = [int(a) for a in prefix]
        self.pts = points_of(p, self.acts)
        assert len(set(self.pts)) == len(self.pts)
        self.on = set(self.pts)
        self.root_len = len(self.pts)
        self.next = 0
        self.leaf = False                   # the current node is an entered leaf
        self.counts = dict.fromkeys(COUNTERS, 0)
        self.first, self.leaves = None, {}
        self.complete = False
        self.path = list(self.acts)
        self.started = False
        # with ``trace``: entry n = (the eight counters, the action bytes) after n entered nodes
        self.trace = [(tuple(self.counts.values()), bytes(self.acts))] if trace else None

    # ------------------------------------------------------------------ the tree
    def _forward(self, frm=0):
        x, y = self.pts[-1]
        out = []
        for a in range(frm, 4):
            nx, ny = x + DIRS[a][0], y + DIRS[a][1]
            if 0 <= nx < self.X and 0 <= ny < self.Y and self.gaps[nx, ny] == 0 and (nx, ny) not in self.on:
                out.append(a)
        return out

    def _pop_legal(self):
        return len(self.pts) >= 2 and self.gaps[self.pts[-2]] == 0

    def _audit(self):
        key = (id(self.p), tuple(self.acts), self.searches)
        hit = Walker._audits.get(key)
        if hit is None:
            pts = [list(pt) for pt in self.pts]
            status = rules_ref.audit(dict(self.p), pts, self.pts[-1])
            hit = {"bits": rules_ref.rule_bits(status), "listed": tuple(self.pts) in self.listed, "searched": None}
            if self.searches:
                from tiling_pools import count_searches
                hit["searched"] = len(count_searches(dict(self.p), pts, self.pts[-1], count=False)) > 0
            hit["puzzle"] = self.p                    # keeps the dict, and so its id, alive
            Walker._audits[key] = hit
        return hit

    def _enter(self, a):
        x, y = self.pts[-1]
        pt = (x + DIRS[a][0], y + DIRS[a][1])
        self.pts.append(pt), self.acts.append(a), self.on.add(pt)
        c = self.counts
        c["nodes"] += 1
        step = self.root_step + len(self.pts) - self.root_len
        self.leaf = True
        if pt == self.target:                                                    # 1192; clears a truncation (1198)
            leaf = self._audit()
            self.leaves[tuple(self.acts)] = leaf
            c["targets"] += 1
            c["listed"] += leaf["listed"]
            if self.undecided is not None and self.undecided(leaf):
                c["undecided"] += 1
            elif leaf["bits"] & RULE_ALL:
                c["satisfied"] += 1
                c["both"] += leaf["listed"]
                if self.first is None:
                    self.first = list(self.acts)
        elif step >= self.max_steps or (not self._forward() and not self._pop_legal()):
            c["truncated"] += 1                                                  # 1134, 1195
        elif not self._forward():
            c["dead_ends"] += 1
        else:
            self.leaf = False
        if self.trace is not None:
            self.trace.append((tuple(c.values()), bytes(self.acts)))

    def _undo(self):
        a = self.acts.pop()
        self.on.remove(self.pts.pop())
        self.leaf = False
        self.next = a + 1

    # ------------------------------------------------------------------ the walk
    def run(self, budget=None):
        """Enter at most ``budget`` more nodes (None: all).  Returns ``self``."""
        if self.complete:
            return self
        if not self.started:
            self.started = True
            if not self._forward():                   # a live root without a forward move: one dead end
                self.counts["dead_ends"] += 1
                self.complete = True
                return self
        entered = 0
        stored = None
        while True:
            cand = [] if self.leaf else self._forward(self.next)
            if cand:
                if budget is not None and entered >= budget:
                    break                             # more to walk: the last entered node stands
                self._enter(cand[0])
                self.next = 0
                entered += 1
                if budget is not None and entered >= budget:
                    stored = (list(self.acts), list(self.pts), self.leaf)
            elif len(self.pts) <= self.root_len:
                self.complete = True
                stored = None
                break
            else:
                self._undo()
        if stored is not None:                        # back to the last entered node
            self.acts, self.pts, self.leaf = stored
            self.on = set(self.pts)
            self.next = 0
        self.path = list(self.acts)
        return self


def walk(p, prefix=(), budget=None, **kw):
    """One ``Walker.run``: the complete walk below ``prefix``, or its first ``budget`` nodes."""
    return Walker(p, prefix, **kw).run(budget)


# ---------------------------------------------------------------- the pools of the tests, built once per process
_pools = {}


def pool(name):
    """Processed puzzles of pool ``name``: "A" 5 x 5 and 7 x 7 lattices (one word), "B" 9 x 9 (two
    words), "C" the first 8 two-walled 15 x 15 puzzles of test_gpu_rules_records' queue test (four)."""
    if name not in _pools:
        from sparc_gym_amd import synthetic
        from sparc_gym_amd.puzzles import process_puzzles
        if name == "A":
            recs = synthetic.make_rule_puzzles(8, seed=6, sizes=((2, 2), (3, 3)), break_prob=0.3)
        elif name == "B":
            recs = synthetic.make_rule_puzzles(4, seed=6, sizes=((4, 4),), break_prob=0.3)
        else:
            from test_gpu_rules_limits import _two_walls
            recs = [r for r in map(_two_walls, synthetic.make_puzzles(200, seed=41, sizes=((7, 7),),
                                                                        full_properties=False, n_solutions=1))
                    if r is not None][:8]
        _pools[name] = process_puzzles(recs)
    return _pools[name]


_walks = {}


def complete_walks(name, **kw):
    """The traced complete walk from the start of every puzzle of pool ``name`` (cached)."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _walks:
        _walks[key] = [Walker(p, trace=True, **kw).run() for p in pool(name)]
    return _walks[key]
