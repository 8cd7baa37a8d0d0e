"""The CPU side of the pruned depth-first search tests (tests/dfs_prune_ref.py), without a GPU: the
consequences of the definition that sparc_dfs_pruned_device states as facts, pinned on the pruned
walker against the unpruned one (tests/dfs_ref.py) on pools A and B from the reset state, and the
pruned walker's own consistency under a budget."""
import pytest

import dfs_prune_ref
import dfs_ref
from dfs_prune_ref import DEADLINE, REACH

TARGET_KEYS = ("targets", "satisfied", "listed", "both", "undecided")
MAX_STEPS = {"A": 64, "B": 128}                                     # as tests/test_gpu_dfs.py: one cache for both


@pytest.fixture(scope="module")
def walks_b():
    """Pool B's complete walks, unpruned and pruned: the slow part, once."""
    return (dfs_ref.complete_walks("B", max_steps=MAX_STEPS["B"]),
            dfs_prune_ref.complete_walks("B", prune=REACH, max_steps=MAX_STEPS["B"]))


def check_same_answer(full, cut):
    for f, c in zip(full, cut):
        assert f.complete and c.complete
        for k in TARGET_KEYS:
            assert c.counts[k] == f.counts[k], k
        assert c.first == f.first
        assert list(c.leaves) == list(f.leaves)                     # the same target leaves in the same order
        assert c.counts["nodes"] <= f.counts["nodes"]
        assert c.counts["dead_ends"] == (1 if c.counts["nodes"] == 0 else 0)   # none below the root
        assert len(c.trace) == c.counts["nodes"] + 1


def test_pool_a_reach():
    full = dfs_ref.complete_walks("A", searches=True, max_steps=MAX_STEPS["A"])
    cut = dfs_prune_ref.complete_walks("A", prune=REACH, searches=True, max_steps=MAX_STEPS["A"])
    check_same_answer(full, cut)
    assert all(c.counts["nodes"] > 0 for c in cut)
    assert sum(c.counts["nodes"] for c in cut) < 0.6 * sum(f.counts["nodes"] for f in full)   # the cut is real
    assert all(c.counts["truncated"] <= f.counts["truncated"] for f, c in zip(full, cut))


def test_pool_b_reach(walks_b):
    full, cut = walks_b
    check_same_answer(full, cut)
    ratio = [f.counts["nodes"] / c.counts["nodes"] for f, c in zip(full, cut)]
    assert min(ratio) > 2.0                                         # about 2.4 to 2.9 on 9 x 9


@pytest.mark.parametrize("max_steps,root_step", [(6, 0), (9, 0), (14, 0), (12, 3)])
def test_pool_a_deadline(max_steps, root_step):
    proc = dfs_ref.pool("A")
    kw = dict(max_steps=max_steps, root_step=root_step, trace=True)
    full = [dfs_ref.Walker(p, **kw).run() for p in proc]
    reach = [dfs_prune_ref.PrunedWalker(p, prune=REACH, **kw).run() for p in proc]
    cut = [dfs_prune_ref.PrunedWalker(p, prune=DEADLINE, **kw).run() for p in proc]
    check_same_answer(full, reach)
    check_same_answer(full, cut)
    assert any(f.counts["truncated"] for f in full) and any(r.counts["truncated"] for r in reach)
    for r, c in zip(reach, cut):
        assert c.counts["truncated"] == 0 and c.counts["nodes"] <= r.counts["nodes"]
        # every entered node lies on a path that reaches the target in time: the walk is the union of
        # the prefixes of the target paths
        prefixes = {a[:k] for a in c.leaves for k in range(1, len(a) + 1)}
        assert c.counts["nodes"] == len(prefixes)
        assert {bytes(t[1]) for t in c.trace[1:]} == {bytes(a) for a in prefixes}
    if max_steps == 6:
        assert any(c.counts["nodes"] == 0 and c.counts["dead_ends"] == 1 for c in cut)   # cut off by the limit


@pytest.mark.parametrize("prune", [REACH, DEADLINE])
@pytest.mark.parametrize("budget", [1, 7, 1000])
def test_budgeted_prefixes_add_up_to_the_complete_pruned_walk(prune, budget):
    ms = MAX_STEPS["A"] if prune == REACH else 14
    for p in dfs_ref.pool("A"):
        full = dfs_prune_ref.PrunedWalker(p, prune=prune, max_steps=ms, trace=True).run()
        total = full.counts["nodes"]
        w = dfs_prune_ref.PrunedWalker(p, prune=prune, max_steps=ms)
        calls = 0
        while not w.complete:
            w.run(budget)
            calls += 1
            k = min(calls * budget, total)
            assert tuple(w.counts.values()) == full.trace[k][0] and w.counts["nodes"] == k
            if not w.complete:
                assert bytes(w.path) == full.trace[k][1] and k == calls * budget < total
        assert calls == max(1, -(-total // budget))                 # complete in the call that enters the last node
        assert w.counts == full.counts and w.first == full.first and w.path == []


def test_the_prune_argument_of_python():
    """What SPaRCVecEnv.dfs and search.solve_dfs_pruned accept, checked before anything touches a device."""
    from sparc_gym_amd import _lib
    assert [_lib.dfs_prune_mode(v) for v in (False, True, "reach", "deadline")] == [0, 1, 1, 3]
    assert (_lib.DFS_PRUNE_REACH, _lib.DFS_PRUNE_DEADLINE, _lib.DFS_STATE_MODE_SHIFT) == (REACH, 2, 12)
    assert DEADLINE == _lib.DFS_PRUNE_REACH | _lib.DFS_PRUNE_DEADLINE
    for bad in (None, 0, 1, 2, 3, -1, "both", "", 1.0):
        with pytest.raises(ValueError, match="prune must be"):
            _lib.dfs_prune_mode(bad)


def test_a_budget_can_end_where_every_remaining_sibling_is_dead():
    """The case the kernel's look-ahead has to get right: after the n-th node of the pruned walk
    the unpruned walker would still find a forward move on the way back up, the pruned one none."""
    found = 0
    for p, cut in zip(dfs_ref.pool("A"), dfs_prune_ref.complete_walks("A", prune=REACH, searches=True,
                                                                         max_steps=MAX_STEPS["A"])):
        total = cut.counts["nodes"]
        w = dfs_prune_ref.PrunedWalker(p, prune=REACH, max_steps=MAX_STEPS["A"]).run(total)
        assert w.complete                                           # the last node's call completes
        acts = list(cut.trace[total][1])
        u = dfs_ref.Walker(p, acts, max_steps=MAX_STEPS["A"])        # stand on that node, look back up unpruned
        u.root_len, u.leaf = 1, True
        while len(u.pts) > 1 and not found:
            u._undo()
            found += bool(u._forward(u.next))
    assert found
