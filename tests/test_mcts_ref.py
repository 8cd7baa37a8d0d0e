"""The UCT model of tests/mcts_ref.py, pinned without a GPU: the invariants every tree it builds must
hold, the resume promise, FULL, greedy selection under an all-zero child table and the clamp of the
table index.  tests/test_gpu_mcts.py compares SPaRCVecEnv.mcts with this model byte for byte."""
import functools

import numpy as np
import pytest

import mcts_ref as ref
from mcts_ref import CHILD, CHILD_WINS, DEAD, INNER, LOSSES, N, NONE, TERMINATED, TRUNCATED, VISITS, WINS
from sparc_gym_amd import synthetic
from sparc_gym_amd.puzzles import process_puzzles

MAX_STEPS, M, SIMS, L = 12, 24, 40, 6


@functools.lru_cache(maxsize=None)
def _pool():
    proc = process_puzzles(synthetic.make_puzzles(64, seed=0, sizes=((3, 3),), full_properties=True))
    return [ref.pool_entry(p) for p in proc]


@functools.lru_cache(maxsize=None)
def _starts(tb):
    return ref.prefixes(_pool(), M, tb, MAX_STEPS, seed=5)


def _run(tb, sims=SIMS, cap=SIMS + 1, tables=None, forward_only=None, **kw):
    ep, ec = ref.uct_tables() if tables is None else tables
    forward_only = tb if forward_only is None else forward_only
    return ref.search(_pool(), _starts(tb), tb, MAX_STEPS, sims, L, cap, ep, ec, seed=3, forward_only=forward_only, **kw)


@functools.lru_cache(maxsize=None)
def _standing(tb):
    return _run(tb)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.status == y.status and x.nodes == y.nodes
        assert (x.win_steps, x.win_actions) == (y.win_steps, y.win_actions)


def test_the_starts_cover_every_status_and_kind():
    """Pending, walled-in and live roots, and under the live ones every kind of node: by
    construction (mcts_ref.prefixes), checked here on what the model reports."""
    for tb in (True, False):
        trees = _standing(tb)
        status = {t.status for t in trees}
        assert status == ({ref.DONE, ref.PENDING, ref.DEAD_END} if tb else {ref.DONE, ref.PENDING})
        kinds = {n[0] >> 30 for t in trees for n in t.nodes}
        assert kinds == ({INNER, TERMINATED, TRUNCATED, DEAD} if tb else {INNER, TERMINATED, TRUNCATED})
        assert any(t.win_actions is not None for t in trees) and any(t.win_actions is None for t in trees)
        for t in trees:
            if t.status != ref.DONE:
                assert t.nodes == [] and t.sims == 0 and t.win_steps == NONE


@pytest.mark.parametrize("tb", [True, False])
def test_invariants_of_every_tree(tb):
    for t in _standing(tb):
        if t.status != ref.DONE:
            continue
        nodes = t.nodes
        assert t.sims == SIMS and nodes[0][VISITS] == SIMS          # root visits = simulations done
        assert len(nodes) <= SIMS + 1                               # one new node per simulation at most
        assert nodes[0][0] == 0                                     # the root: parent 0, action 0, inner
        for i, n in enumerate(nodes):
            kind = n[0] >> 30
            tried = [a for a in range(4) if n[CHILD + a] not in (0, NONE)]
            edge_n, edge_w = sum(n[N + a] for a in range(4)), sum(n[CHILD_WINS + a] for a in range(4))
            if i == 0:
                # every simulation leaves the root through an edge
                assert n[VISITS] == edge_n and n[WINS] == edge_w
            elif kind == INNER:
                # the simulation that created the node rolled out from it; every later one that
                # came through left it through an edge
                assert n[VISITS] == 1 + edge_n and n[WINS] - edge_w in (0, 1)
            else:
                # an end node: every visit ends on it with the same step, so with the same code
                assert tried == [] and edge_n == 0 and all(n[CHILD + a] == NONE for a in range(4))
                assert n[WINS] in (0, n[VISITS]) and n[LOSSES] in (0, n[VISITS])
                if kind == DEAD:
                    assert n[WINS] == 0
            assert n[WINS] + n[LOSSES] <= n[VISITS] and n[VISITS] >= 1
            for a in range(4):
                c = n[CHILD + a]
                if c in (0, NONE):
                    assert n[N + a] == 0 and n[CHILD_WINS + a] == 0
                else:
                    # the edge's counters are the child's own words; the links point both ways
                    assert i < c < len(nodes)
                    assert nodes[c][0] & 0x0FFFFFFF == i and (nodes[c][0] >> 28) & 3 == a
                    assert n[N + a] == nodes[c][VISITS] and n[CHILD_WINS + a] == nodes[c][WINS]
            # the lowest untried action goes first: no tried child lies above an untried one
            untried = [a for a in range(4) if n[CHILD + a] == 0]
            assert not untried or not tried or max(tried) < min(untried)
        if t.win_actions is not None:
            assert t.win_steps == len(t.win_actions) >= 1
            assert nodes[0][WINS] >= 1


@pytest.mark.parametrize("tb", [True, False])
def test_split_calls_give_the_same_tree(tb):
    trees = None
    for part in (7, 13, 20):
        trees = _run(tb, sims=part, trees=trees)
        assert all(t.sims == part for t in trees if t.status == ref.DONE)
    _same(trees, _standing(tb))


def test_a_full_arena_stops_before_anything_is_counted():
    cap = 9
    small = _run(True, cap=cap)
    assert {t.status for t in small} >= {ref.FULL}
    for t, whole in zip(small, _standing(True)):
        if t.status != ref.FULL:
            continue
        assert len(t.nodes) == cap and t.sims >= cap - 1 and t.nodes[0][VISITS] == t.sims
        # what it holds is what a search of t.sims simulations on an ample arena holds
        again = ref.Tree(t.root).run(t.sims, L, SIMS + 1, *ref.uct_tables(), seed=3,
                                     id_base=small.index(t) << 32, forward_only=True)
        assert again.status == ref.DONE and again.nodes == t.nodes and again.win_actions == t.win_actions
        # and the search goes on from there on a larger arena
        t.run(SIMS - t.sims, L, SIMS + 1, *ref.uct_tables(), seed=3, id_base=small.index(t) << 32, forward_only=True)
        assert t.status == ref.DONE and t.nodes == whole.nodes and t.win_actions == whole.win_actions
    one = _run(True, cap=1)
    for t in one:
        if t.status == ref.FULL:
            assert t.sims == 0 and len(t.nodes) == 1 and t.nodes[0][VISITS] == 0
    assert {t.status for t in one} == {ref.FULL, ref.PENDING, ref.DEAD_END}


def test_an_all_zero_child_table_is_greedy_selection():
    """ec = 0: the exploration term is +0 whatever ep says, so the choice is the best win rate."""
    ep, _ = ref.uct_tables(3.0)
    zero = np.zeros_like(ep)
    greedy = _run(True, tables=(ep, zero))
    _same(greedy, _run(True, tables=(zero, zero)))
    differs = any(g.nodes != u.nodes for g, u in zip(greedy, _standing(True)))
    assert differs                                                  # exploration does change the trees


def test_table_indices_clamp_at_the_last_entry():
    short = (np.array([0.3, 1.1], np.float32), np.array([1.0, 0.6], np.float32))
    filled = tuple(np.concatenate([t, np.full(62, t[1], np.float32)]) for t in short)
    _same(_run(True, tables=short), _run(True, tables=filled))
    with pytest.raises(AssertionError):
        _run(True, tables=(short[0][:1], short[1][:1]))
