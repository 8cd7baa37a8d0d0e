"""The CPU side of the depth-first search tests (tests/dfs_ref.py), without a GPU: the facts about
the three pools that make the GPU comparison meaningful, and the walker's own consistency: its
budgeted prefixes add up to its complete walk."""
import pytest

import dfs_ref
from record_path import DIRS
from sparc_gym_amd.puzzles import pack_table

RULE_ALL = dfs_ref.RULE_ALL


def _walk_counts(walks, key):
    return [w.counts[key] for w in walks]


def test_pool_a_facts():
    proc = dfs_ref.pool("A")
    walks = dfs_ref.complete_walks("A", searches=True)
    assert {(p["x_size"], p["y_size"]) for p in proc} == {(5, 5), (7, 7)}
    assert pack_table(proc).words == 1
    targets = _walk_counts(walks, "targets")
    assert min(targets) == 8 and max(targets) == 178 and sum(targets) == 613
    assert all(w.complete and len(w.leaves) == w.counts["targets"] >= 1 for w in walks)
    bits = [leaf["bits"] for w in walks for leaf in w.leaves.values()]
    assert any(b & RULE_ALL for b in bits) and any(not b & RULE_ALL for b in bits)
    searched = [sum(leaf["searched"] for leaf in w.leaves.values()) for w in walks]
    assert searched == [0, 0, 0, 0, 110, 0, 5, 34]
    assert sum(bool(leaf["searched"] and leaf["bits"] & RULE_ALL) for w in walks for leaf in w.leaves.values()) == 4
    for w in walks:                                                # the counters hang together
        c = w.counts
        assert c["satisfied"] == sum(bool(leaf["bits"] & RULE_ALL) for leaf in w.leaves.values())
        assert c["listed"] == sum(leaf["listed"] for leaf in w.leaves.values())
        assert c["targets"] + c["dead_ends"] + c["truncated"] <= c["nodes"] and c["undecided"] == 0
        assert len(w.trace) == c["nodes"] + 1 and w.trace[-1][0] == tuple(c.values())
        sat = sorted(a for a, leaf in w.leaves.items() if leaf["bits"] & RULE_ALL)
        assert w.first == (list(sat[0]) if sat else None)          # pre-order = lexicographic order
    assert any(w.first is None for w in walks) and any(w.counts["both"] for w in walks)


def test_pool_b_facts():
    proc = dfs_ref.pool("B")
    walks = dfs_ref.complete_walks("B")
    assert {(p["x_size"], p["y_size"]) for p in proc} == {(9, 9)}
    assert pack_table(proc).words == 2
    assert _walk_counts(walks, "targets") == [3799, 4294, 5489, 4294]
    assert sum(_walk_counts(walks, "satisfied")) == 66


def _solution_actions(p):
    sp = p["solution_paths"][0]
    return [DIRS.index((int(b[0]) - int(a[0]), int(b[1]) - int(a[1]))) for a, b in zip(sp[:-1], sp[1:])]


def pool_c_roots():
    """(puzzle, prefix actions) of pool C's 16 roots: each puzzle's first solution cut 4 and 10
    moves before its end."""
    out = []
    for q, p in enumerate(dfs_ref.pool("C")):
        sol = _solution_actions(p)
        out += [(q, sol[:len(sol) - cut]) for cut in (4, 10)]
    return out


def test_pool_c_facts():
    proc = dfs_ref.pool("C")
    assert len(proc) == 8 and pack_table(proc).words == 4
    assert {(p["x_size"], p["y_size"]) for p in proc} == {(15, 15)}
    walks = [dfs_ref.walk(proc[q], pre, budget=3000, root_step=len(pre), max_steps=256) for q, pre in pool_c_roots()]
    assert sum(w.complete for w in walks) == 12 and sum(not w.complete for w in walks) == 4
    assert all(w.counts["nodes"] == 3000 for w in walks if not w.complete)
    assert max(_walk_counts(walks, "targets")) == 198


@pytest.mark.parametrize("budget", [1, 7, 1000])
def test_budgeted_prefixes_add_up_to_the_complete_walk(budget):
    for p, full in zip(dfs_ref.pool("A"), dfs_ref.complete_walks("A", searches=True)):
        total = full.counts["nodes"]
        w = dfs_ref.Walker(p, searches=True)
        calls = 0
        while not w.complete:
            w.run(budget)
            calls += 1
            k = min(calls * budget, total)
            assert tuple(w.counts.values()) == full.trace[k][0]
            assert w.counts["nodes"] == k
            if not w.complete:
                assert bytes(w.path) == full.trace[k][1] and k == calls * budget < total
        assert calls == -(-total // budget)                        # complete in the call that enters the last node
        assert w.counts == full.counts and w.first == full.first and w.path == []
        assert list(w.leaves) == list(full.leaves)
        assert w.run(budget).counts == full.counts                 # one more call adds nothing


def test_walk_below_a_prefix_and_a_root_dead_end():
    p = dfs_ref.pool("A")[3]
    full = dfs_ref.complete_walks("A", searches=True)[3]
    # the subtrees below the root's children partition the tree
    first = sorted({a[0] for a in full.leaves})
    subs = [dfs_ref.walk(p, [a], searches=True) for a in range(4) if any(t[1][:1] == bytes([a]) for t in full.trace)]
    assert len(subs) >= len(first) >= 1
    assert sum(s.counts["nodes"] for s in subs) + len(subs) == full.counts["nodes"]
    assert sum(s.counts["targets"] for s in subs) == full.counts["targets"]
    # a prefix that has walked itself into a corner: a live root without a forward move
    dead = next(t[1] for k, t in enumerate(full.trace[1:], 1)
                if t[0][5] == full.trace[k - 1][0][5] + 1)             # the node that raised dead_ends
    w = dfs_ref.walk(p, list(dead))
    assert w.complete and w.counts == dict(dfs_ref.Walker(p).counts, dead_ends=1)
