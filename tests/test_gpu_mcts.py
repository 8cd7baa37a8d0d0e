"""UCT tree search of state records on the GPU (SPaRCVecEnv.mcts, sparc_mcts_device).

The yardstick is the model of tests/mcts_ref.py (pinned on the CPU by tests/test_mcts_ref.py): the
same search over the CPU restatement of the env, with search.rand_pick and numpy float32 scores.
Everything the call returns is compared with it byte for byte: the arena, count, status, sims,
win_steps, and win through ``replay`` of the model's winning actions.  The roots are the mid-episode
starts of ``mcts_ref.prefixes`` on the standing pools of test_gpu_snapshot.py (max_steps 12), made
into records by ``replay``: of every eight, five live ones, one two steps short of the limit (the
step limit truncates inside its tree), one pending and one walled in.  Checks that do not use the
model follow: one simulation against ``expand`` + ``playout``, the winner against ``replay``, the
node count against ``dfs``."""
import ctypes
import functools

import numpy as np
import pytest

import mcts_ref as ref
from sparc_gym_amd import _lib
from test_gpu_snapshot import MAX_STEPS, _tables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 3
NODE = _lib.MCTS_NODE_WORDS
# name, traceback, M, sims, L, cap, forward_only.  M: one lane; a wave and a lane; a workgroup and a
# lane.  L = 1: every rollout is one step.  cap 1: FULL before the first simulation; cap 2: one node.
CASES = [
    ("7x7_full", True, 257, 40, 6, 41, True),
    ("7x7_full", True, 65, 40, 6, 41, False),
    ("7x7_full", False, 65, 40, 6, 41, False),
    ("7x7_full", False, 65, 40, 6, 41, True),
    ("mixed_5_11", True, 65, 40, 6, 41, True),
    ("15x15", True, 65, 40, 6, 41, True),
    ("7x7_full", True, 1, 1, 1, 2, True),
    ("7x7_full", True, 65, 1, 6, 2, True),
    ("7x7_full", True, 65, 40, 1, 41, True),
    ("7x7_full", True, 65, 40, 6, 1, True),
    ("7x7_full", True, 65, 40, 6, 2, True),
    ("7x7_full", True, 65, 40, 6, 9, True),
]


def _vec(name, tb):
    from sparc_gym_amd import SPaRCVecEnv
    proc, table, _ = _tables(name)
    return SPaRCVecEnv(4, processed=proc, table=table, traceback=tb, max_steps=MAX_STEPS, autoreset="none",
                       observation="compact")


@functools.lru_cache(maxsize=None)
def _pool(name):
    return [ref.pool_entry(p) for p in _tables(name)[0]]


@functools.lru_cache(maxsize=None)
def _starts(name, tb, M):
    return ref.prefixes(_pool(name), M, tb, MAX_STEPS, seed=5)


def _pad(lists):
    """action lists as replay's [L, M] uint8 and lengths (None for L = 0)"""
    L = max((len(a) for a in lists), default=0)
    if L == 0:
        return None, None
    acts = np.full((L, len(lists)), 255, np.uint8)
    for j, a in enumerate(lists):
        acts[:len(a), j] = a
    return acts, np.array([len(a) for a in lists], np.int64)


def _roots(v, name, tb, M):
    """the starts as records: replay of each prefix from its puzzle's reset state"""
    starts = _starts(name, tb, M)
    acts, lens = _pad([a for _, a in starts])
    pids = np.array([p for p, _ in starts], np.int64)
    return v.replay(puzzle_indices=pids, actions=acts, lengths=lens)["final"]


@functools.lru_cache(maxsize=None)
def _model(name, tb, M, parts, L, caps, forward, id0=0):
    """the model's trees after calls of ``parts`` simulations on arenas of ``caps`` nodes"""
    trees = None
    for sims, cap in zip(parts, caps):
        trees = ref.search(_pool(name), _starts(name, tb, M), tb, MAX_STEPS, sims, L, cap, *ref.uct_tables(),
                           seed=SEED, id0=id0, forward_only=forward, trees=trees)
    return trees


def _check(v, snap, out, trees, cap, sims=None):
    """everything ``out`` holds against the model's ``trees``"""
    M = len(trees)
    assert out["nodes"].shape == (M, cap, NODE) and out["nodes"].dtype == torch.uint32 and out["nodes"].is_cuda
    assert out["count"].dtype == torch.int32 and out["status"].dtype == torch.uint8
    assert np.array_equal(out["status"].cpu().numpy(), [t.status for t in trees])
    assert np.array_equal(out["sims"].cpu().numpy(), [t.sims for t in trees] if sims is None else sims)
    assert np.array_equal(out["count"].cpu().numpy(), [len(t.nodes) for t in trees])
    got = out["nodes"].cpu().numpy()
    for j, t in enumerate(trees):
        assert np.array_equal(got[j], t.array(cap)), f"the tree of root {j}"
    want = np.array([-1 if t.win_actions is None else t.win_steps for t in trees], np.int64)
    assert np.array_equal(out["win_steps"].cpu().numpy(), want)
    win = out["win"].records.cpu().numpy()
    assert not win[want < 0].any()
    acts, lens = _pad([t.win_actions or [] for t in trees])
    if acts is not None:
        # the model's winning actions, played from the roots by the replay kernel
        fin = v.replay(snap, acts, lengths=lens, stop_done=True)
        assert np.array_equal(fin["final"].records.cpu().numpy()[want >= 0], win[want >= 0])
        assert (fin["reward_code"].cpu().numpy()[want >= 0] == 100).all()
    v.core.sync()


# ----------------------------------------------------------------------------- 1. the model
@pytest.mark.parametrize("name,tb,M,sims,L,cap,forward", CASES)
def test_trees_equal_the_model(on_gpu, name, tb, M, sims, L, cap, forward):
    v = _vec(name, tb)
    snap = _roots(v, name, tb, M)
    trees = _model(name, tb, M, (sims,), L, (cap,), forward)
    status = {t.status for t in trees}
    if M >= 65:
        # on the model's own results: the roots show what they were made to show
        assert ref.PENDING in status
        if cap >= sims + 1:
            assert ref.DONE in status and ref.FULL not in status
        else:
            assert ref.FULL in status
        if name == "7x7_full":
            assert (ref.DEAD_END in status) == tb
            if cap > sims > 1:
                assert {n[0] >> 30 for t in trees for n in t.nodes} >= {ref.INNER, ref.TERMINATED, ref.TRUNCATED}
    if cap == 1:
        assert all(t.sims == 0 for t in trees) and ref.DONE not in status
    out = v.mcts(snap, sims, L, cap=cap, seed=SEED, forward_only=forward)
    _check(v, snap, out, trees, cap)


def test_default_arguments(on_gpu):
    """cap defaults to sims + 1, forward_only to the env's traceback, the tables to uct_tables(c)."""
    from sparc_gym_amd.vec_env import uct_tables
    for a, b in zip(uct_tables(0.5, 64), ref.uct_tables(0.5, 64)):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    name, tb, M, sims, L = "7x7_full", True, 65, 40, 6
    v = _vec(name, tb)
    snap = _roots(v, name, tb, M)
    out = v.mcts(snap, sims, L, seed=SEED)
    _check(v, snap, out, _model(name, tb, M, (sims,), L, (sims + 1,), True), sims + 1)
    # explore= overrides c; an id0 past 2^63 and a seed change the draws
    ep, ec = ref.uct_tables(1.0)
    again = v.mcts(snap, sims, L, c=7.0, explore=(ep, torch.from_numpy(ec)), seed=SEED)
    assert torch.equal(again["nodes"].view(torch.int32), out["nodes"].view(torch.int32))
    id0 = 2**63 + 5
    far = v.mcts(snap, sims, L, seed=SEED, id0=id0)
    _check(v, snap, far, _model(name, tb, M, (sims,), L, (sims + 1,), True, id0), sims + 1)
    assert not torch.equal(far["nodes"].view(torch.int32), out["nodes"].view(torch.int32))


# ----------------------------------------------------------------------------- 2. without the model
def _forward_masks(v, snap):
    """(expand's result, the forward moves of every record): its legal actions without the traceback
    pop, the pop being the child one point shorter than its parent"""
    ex = v.expand(snap)
    M = len(snap)
    legal = ex["legal_mask"].cpu().numpy().astype(np.int64)
    shorter = (ex["children"].fields()["path_len"].reshape(M, 4) < snap.fields()["path_len"][:, None]).cpu().numpy()
    return ex, legal & ~(shorter * (1 << np.arange(4))).sum(1)


def test_one_simulation_is_expand_and_one_playout(on_gpu):
    """sims = 1: node 1 is the ``expand`` child of the lowest forward action, and its statistics are
    those of ``playout(K=1)`` from that child with the same seed, id, horizon and flag."""
    name, M, L = "7x7_full", 65, 6
    for tb, forward in ((True, True), (True, False), (False, False)):
        v = _vec(name, tb)
        snap = _roots(v, name, tb, M)
        out = v.mcts(snap, 1, L, seed=SEED, forward_only=forward)
        nodes = out["nodes"].cpu().numpy().astype(np.int64)
        status = out["status"].cpu().numpy()
        ex, fwd = _forward_masks(v, snap)
        fwd2 = _forward_masks(v, ex["children"])[1].reshape(M, 4)          # of every child
        pend = (snap.numpy()[:, 6] >> 2) & 1 != 0
        assert np.array_equal(status == _lib.MCTS_PENDING, pend)
        assert np.array_equal(status == _lib.MCTS_DEAD_END, ~pend & (fwd == 0))
        live = np.nonzero(status == _lib.MCTS_DONE)[0]
        assert len(live) > M // 2 and (out["count"].cpu().numpy()[live] == 2).all()
        code, flags = ex["reward_code"].cpu().numpy(), ex["flags"].cpu().numpy()
        rolled = 0
        for j in live:
            a = int(fwd[j] & -fwd[j]).bit_length() - 1
            root, node = nodes[j, 0], nodes[j, 1]
            kind = 1 if flags[j, a] & 1 else 2 if flags[j, a] & 2 else 3 if fwd2[j, a] == 0 else 0
            want = [_lib.MCTS_NO_CHILD if not (fwd[j] >> b) & 1 else int(b == a) for b in range(4)]
            assert list(root[4:8]) == want and root[0] == 0
            assert node[0] == 0 | (a << 28) | (kind << 30)
            assert list(node[4:8]) == [0 if kind == 0 and (fwd2[j, a] >> b) & 1 else _lib.MCTS_NO_CHILD for b in range(4)]
            last, steps = int(code[j, a]), 1
            if kind == 0:
                child = ex["children"].select([4 * int(j) + a])
                po = v.playout(child, 1, L, seed=SEED, id0=int(j) << 32, forward_only=forward, stats=False)
                assert int(po["steps"][0, 0]) >= 1
                last, steps = int(po["reward_code"][0, 0]), 1 + int(po["steps"][0, 0])
                rolled += 1
            win, loss = int(last == 100), int(last == -100)
            assert list(node[1:4]) == [1, win, loss] and list(root[1:4]) == [1, win, loss]
            assert root[8 + a] == 1 and root[12 + a] == win and root[8:16].sum() == 1 + win
            assert not node[8:16].any()
            assert int(out["win_steps"][j]) == (steps if win else -1)
        assert rolled > len(live) // 2
        v.core.sync()


def test_the_winner_replays_from_the_root(on_gpu):
    """``replay`` of the winner's moves below the root ends with code +100 in ``win_steps`` steps and
    gives ``win`` byte for byte."""
    name, tb, M, sims, L = "7x7_full", True, 257, 40, 6
    v = _vec(name, tb)
    snap = _roots(v, name, tb, M)
    out = v.mcts(snap, sims, L, seed=SEED)
    steps = out["win_steps"].cpu().numpy()
    won = np.nonzero(steps >= 0)[0]
    assert len(won) >= 8
    root_moves, win_moves = snap.moves(), out["win"].moves()
    tails = []
    for j in won:
        assert win_moves[j][:len(root_moves[j])] == root_moves[j]        # forward only: the root's path goes on
        tails.append(win_moves[j][len(root_moves[j]):])
        assert len(tails[-1]) == steps[j]
    acts, lens = _pad(tails)
    fin = v.replay(snap.select(won), acts, lengths=lens)
    assert (fin["reward_code"].cpu().numpy() == 100).all() and (fin["end"].cpu().numpy() == _lib.REPLAY_END_EXHAUSTED).all()
    assert np.array_equal(fin["steps"].cpu().numpy(), steps[won])
    assert torch.equal(fin["final"].records, out["win"].records[torch.as_tensor(won, device="cuda")])
    v.core.sync()


def test_a_tree_never_outgrows_the_forward_tree(on_gpu):
    """count <= the NODES of ``dfs`` + 1 for every root whose walk completes, with equality on the
    roots the search exhausts."""
    name, tb, M, sims, L = "7x7_full", True, 257, 60, 6
    v = _vec(name, tb)
    snap = _roots(v, name, tb, M)
    out = v.mcts(snap, sims, L, seed=SEED)
    walk = v.dfs(snap, 1 << 16)
    done = (walk["status"] == _lib.DFS_COMPLETE).cpu().numpy() & (out["status"].cpu().numpy() == _lib.MCTS_DONE)
    nodes = walk["counts"][:, _lib.DFS_NODES].cpu().numpy()
    count = out["count"].cpu().numpy()
    assert done.sum() >= 16
    assert (count[done] <= nodes[done] + 1).all()
    assert (count[done] == nodes[done] + 1).any() and (count[done] < nodes[done] + 1).any()
    v.core.sync()


# ----------------------------------------------------------------------------- 3. resumable trees
def _equal_trees(a, b):
    for k in ("nodes", "count", "win_steps", "status"):
        x, y = (t[k].view(torch.int32) if t[k].dtype == torch.uint32 else t[k] for t in (a, b))
        assert torch.equal(x, y), k
    assert torch.equal(a["win"].records, b["win"].records)


@pytest.mark.parametrize("name,tb,forward", [("7x7_full", True, True), ("7x7_full", False, False),
                                             ("mixed_5_11", True, False)])
def test_split_calls_equal_one_call(on_gpu, name, tb, forward):
    M, L, cap = 257, 6, 41
    v = _vec(name, tb)
    snap = _roots(v, name, tb, M)
    whole = v.mcts(snap, 40, L, cap=cap, seed=SEED, forward_only=forward)
    tree, total = None, 0
    for part in (7, 13, 20):
        tree = v.mcts(snap, part, L, cap=cap, tree=tree, seed=SEED, forward_only=forward)
        total = total + tree["sims"]
    _equal_trees(tree, whole)
    assert torch.equal(total, whole["sims"])
    v.core.sync()


def test_full_then_a_larger_arena(on_gpu):
    """FULL on 9 nodes, the trees copied into arenas of 81, 40 more simulations: what the model gives
    for the same two calls (that this equals one search on the large arena is pinned on the model)."""
    name, tb, M, L = "7x7_full", True, 65, 6
    v = _vec(name, tb)
    snap = _roots(v, name, tb, M)
    small = v.mcts(snap, 40, L, cap=9, seed=SEED)
    first = _model(name, tb, M, (40,), L, (9,), True)
    assert (small["status"] == _lib.MCTS_FULL).any()
    sims0 = [t.sims for t in first]
    kept = small["nodes"].view(torch.int32).clone()
    grown = v.mcts(snap, 40, L, cap=81, tree=small, seed=SEED)
    assert torch.equal(small["nodes"].view(torch.int32), kept)            # the small arena was copied, not reused
    trees = _model(name, tb, M, (40, 40), L, (9, 81), True)
    _check(v, snap, grown, trees, 81)
    assert [int(t.nodes[0][ref.VISITS]) for t in trees if t.status == ref.DONE] == \
        [s + 40 for s, t in zip(sims0, trees) if t.status == ref.DONE]
    with pytest.raises(ValueError, match="cap"):
        v.mcts(snap, 1, L, cap=80, tree=grown)


# ----------------------------------------------------------------------------- 4. refusals
def test_a_damaged_arena_is_refused_for_that_root_only(on_gpu):
    name, tb, M, L, cap = "7x7_full", True, 65, 6, 41
    v = _vec(name, tb)
    snap = _roots(v, name, tb, M)
    base = v.mcts(snap, 30, L, cap=cap, seed=SEED)
    v.core.sync()
    nodes = base["nodes"].cpu().numpy()
    count = base["count"].cpu().numpy()
    # roots whose every child has been tried and that hold a few nodes: the next simulation descends
    ready = [j for j in range(M) if count[j] >= 6 and not (nodes[j, 0, 4:8] == 0).any()]
    assert len(ready) >= 3
    a, b, c = ready[0], ready[len(ready) // 2], ready[-1]
    bad_nodes, bad_count = nodes.copy(), count.copy()
    real = (bad_nodes[a, 0, 4:8] != 0) & (bad_nodes[a, 0, 4:8] != _lib.MCTS_NO_CHILD)
    bad_nodes[a, 0, 4:8][real] = count[a] + 3                            # child indices >= count
    idx = np.arange(1, count[b], dtype=np.uint32)
    bad_nodes[b, 1:count[b], 0] = (bad_nodes[b, 1:count[b], 0] & 0xF0000000) | idx   # parent = the node itself
    bad_count[c] = cap + 1                                               # count > cap

    def tree_of(n, k):
        return {"nodes": torch.from_numpy(n).cuda(), "count": torch.from_numpy(k).cuda(),
                "win": base["win"].records.clone(), "win_steps": base["win_steps"].clone()}

    good = v.mcts(snap, 10, L, tree=tree_of(nodes.copy(), count.copy()), seed=SEED)
    v.core.sync()
    got = v.mcts(snap, 10, L, tree=tree_of(bad_nodes, bad_count), seed=SEED)
    with pytest.raises(ValueError, match="out of range"):
        v.core.sync()
    v.core.sync()                                                        # reported once
    status = got["status"].cpu().numpy()
    want = good["status"].cpu().numpy().copy()
    want[[a, b, c]] = _lib.MCTS_INVALID
    assert np.array_equal(status, want)
    assert (got["sims"].cpu().numpy()[[a, b, c]] == 0).all()
    out_nodes, out_count = got["nodes"].cpu().numpy(), got["count"].cpu().numpy()
    others = np.setdiff1d(np.arange(M), [a, b, c])
    assert np.array_equal(out_nodes[others], good["nodes"].cpu().numpy()[others])
    assert np.array_equal(out_count[others], good["count"].cpu().numpy()[others])
    assert torch.equal(got["win"].records, good["win"].records)
    # the refused trees stand as they were handed in
    assert np.array_equal(out_nodes[[a, b, c]], bad_nodes[[a, b, c]])
    assert np.array_equal(out_count[[a, b, c]], bad_count[[a, b, c]])
    # a bad root record is refused the same way
    rec = snap.records.clone()
    rec[a, 12:16] = 255                                                  # the puzzle index
    from sparc_gym_amd.snapshot import Snapshot
    refused = v.mcts(Snapshot(rec, snap.info), 10, L, seed=SEED)
    with pytest.raises(ValueError, match="out of range"):
        v.core.sync()
    st = refused["status"].cpu().numpy()
    assert st[a] == _lib.MCTS_INVALID and int(refused["count"][a]) == 0 and not refused["nodes"][a].view(torch.int32).any()
    assert np.array_equal(np.delete(st, a), np.delete([t.status for t in _model(name, tb, M, (10,), L, (11,), True)], a))


def test_bad_arguments_name_the_argument(on_gpu):
    name, tb, M, L = "7x7_full", True, 5, 6
    v = _vec(name, tb)
    snap = _roots(v, name, tb, M)
    ep, ec = ref.uct_tables()
    nan = ep.copy()
    nan[7] = np.nan
    for kw, what in ((dict(sims=0), "sims"), (dict(sims=2**31), "sims"), (dict(horizon=0), "horizon"),
                     (dict(horizon=65536), "horizon"), (dict(cap=0), "cap"), (dict(cap=2**24 + 1), "cap"),
                     (dict(explore=(nan, ec)), "finite"), (dict(explore=(ep, np.full_like(ec, np.inf))), "finite"),
                     (dict(explore=(ep[:5], ec[:6])), "same length"), (dict(explore=(ep[:1], ec[:1])), "T"),
                     (dict(explore=ep), "explore")):
        args = dict(sims=4, horizon=L)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            v.mcts(snap, **args)
    out = v.mcts(snap, 4, L)
    for key, val, what in (("nodes", out["nodes"][:, :, :8], "nodes"), ("nodes", out["nodes"].view(torch.int32), "nodes"),
                           ("count", out["count"][:3], "count"), ("win_steps", out["win_steps"].float(), "win_steps"),
                           ("win", out["win"].records[:, :16], "win")):
        with pytest.raises(ValueError, match=what):
            v.mcts(snap, 4, L, tree={**out, key: val})
    other = _vec(name, False)
    with pytest.raises(ValueError, match="traceback"):
        other.mcts(snap, 4, L)
    # the C entry point checks for itself, before any launch
    lib, ctx, info = v.core.lib, v.core.ctx, snap.info
    o = _lib.SparcMctsOut(*(out[k].data_ptr() for k in ("status", "sims")), out["win"].records.data_ptr(),
                          out["count"].data_ptr())
    tab = torch.zeros(8, dtype=torch.float32, device="cuda")
    ok = dict(rec=snap.records.data_ptr(), M=M, sims=4, L=L, flags=0, ep=tab.data_ptr(), ec=tab.data_ptr(), T=8, cap=5,
              nodes=out["nodes"].data_ptr(), count=out["count"].data_ptr())
    for kw, what in ((dict(sims=0), b"sims"), (dict(L=0), b"L must"), (dict(L=65536), b"L must"), (dict(cap=0), b"cap"),
                     (dict(cap=2**24 + 1), b"cap"), (dict(flags=2), b"flags"), (dict(T=1), b"T must"),
                     (dict(M=0), b"M must"), (dict(ep=None), b"ep"), (dict(nodes=None), b"nodes"),
                     (dict(nodes=out["nodes"].data_ptr() + 16), b"64-B"), (dict(count=None), b"count")):
        a = {**ok, **kw}
        rc = lib.sparc_mcts_device(ctx, ctypes.byref(info), a["rec"], a["M"], a["sims"], a["L"], 0, 0, a["flags"],
                                   a["ep"], a["ec"], a["T"], a["cap"], a["nodes"], a["count"], ctypes.byref(o))
        assert rc == -1 and what in lib.sparc_last_error(ctx), (kw, lib.sparc_last_error(ctx))
    v.core.sync()


# ----------------------------------------------------------------------------- 5. host form, streams
def test_host_form_equals_device_form(on_gpu):
    name, tb, M, L, cap = "mixed_5_11", True, 65, 6, 41
    v = _vec(name, tb)
    snap = _roots(v, name, tb, M)
    dev = v.mcts(snap, 40, L, cap=cap, seed=SEED)
    ep, ec = ref.uct_tables()
    flags = _lib.PLAYOUT_FORWARD
    host = v.core.mcts_host(snap.info, snap.numpy(), 15, L, ep, ec, cap, seed=SEED, flags=flags)
    assert host["sims"].max() == 15
    host = v.core.mcts_host(snap.info, snap.numpy(), 25, L, ep, ec, cap, nodes=host["nodes"], count=host["count"],
                            win=host["win"], win_steps=host["win_steps"], seed=SEED, flags=flags)
    assert np.array_equal(host["nodes"], dev["nodes"].cpu().numpy())
    assert np.array_equal(host["count"], dev["count"].cpu().numpy().astype(np.uint32))
    assert np.array_equal(host["status"], dev["status"].cpu().numpy())
    assert np.array_equal(host["win"], dev["win"].records.cpu().numpy())
    assert np.array_equal(host["win_steps"].astype(np.int32), dev["win_steps"].cpu().numpy().astype(np.int32))


def test_on_a_caller_stream(on_gpu):
    """Two launches, the second continuing the first, behind one gate on a caller's stream (the
    method of test_gpu_streams.py): the true roots reach the records behind the gate, the poison is
    the puzzles' reset states, whose trees differ; outputs are filled with a sentinel behind the gate."""
    from test_gpu_streams import SENT, _Gate
    name, tb, M, L, cap = "7x7_full", True, 257, 6, 41
    trees = _model(name, tb, M, (40,), L, (cap,), True)
    S, X = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(S):
        v = _vec(name, tb)
        roots = _roots(v, name, tb, M)
        poison = v.roots(np.array([p for p, _ in _starts(name, tb, M)], np.int64)).records.clone()
        assert not torch.equal(poison, roots.records)
        info, rb = roots.info, roots.info.record_bytes
        cur = poison.clone()
        ep, ec = (torch.from_numpy(t).cuda() for t in ref.uct_tables())
        nodes = torch.zeros((M, cap, NODE), dtype=torch.int32, device="cuda")
        count = torch.zeros(M, dtype=torch.int32, device="cuda")
        win = torch.zeros((M, rb), dtype=torch.uint8, device="cuda")
        wsteps = torch.full((M,), -1, dtype=torch.int32, device="cuda")
        status = torch.empty((2, M), dtype=torch.uint8, device="cuda")
        done = torch.empty((2, M), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        assert v._bound_stream == S.cuda_stream
        g = _Gate(S)
        cur.copy_(roots.records, non_blocking=True)
        status.fill_(SENT)
        done.fill_(SENT)
        for k, part in enumerate((15, 25)):
            v.core.mcts_device(info, cur.data_ptr(), M, part, L, ep.data_ptr(), ec.data_ptr(), len(ep), cap,
                               nodes.data_ptr(), count.data_ptr(), status[k].data_ptr(), done[k].data_ptr(),
                               win.data_ptr(), wsteps.data_ptr(), seed=SEED, flags=_lib.PLAYOUT_FORWARD)
        g.assert_closed("two mcts_device launches")
        kept = [t.clone() for t in (nodes, count, win, wsteps, status, done)]
    S.synchronize()
    from sparc_gym_amd.snapshot import Snapshot
    out = {"nodes": kept[0].view(torch.uint32), "count": kept[1], "win": Snapshot(kept[2], info),
           "win_steps": kept[3].to(torch.int64), "status": kept[4][1], "sims": kept[5][0] + kept[5][1]}
    with torch.cuda.stream(S):
        _check(v, roots, out, trees, cap)
    # the method binds the stream it is called on
    X.wait_stream(S)
    with torch.cuda.stream(X):
        v.mcts(roots, 2, L)
        assert v._bound_stream == X.cuda_stream
        v.core.sync()
