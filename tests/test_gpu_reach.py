"""Target reachability and distance maps of state records on the GPU (SPaRCVecEnv.reach,
search.expand_frontier / solve_by_rules with prune, sparc_reach_records_device / _host).

Yardsticks: tests/reach_ref.py, the breadth-first search written from the definition (pinned on
hand-made boards by tests/test_reach_ref.py, which also asserts the coverage of the fixture used
here), on the C oracle's state after step 20 of the geometry pools' standing trace; the kernels the
project already has, on the same records (observe, expand, dfs); and a CPU walk of the forward-move
tree for the pruned search.  Every comparison is exact."""
import copy
import ctypes
import functools

import numpy as np
import pytest

import dfs_ref
import geometry_pools as gp
import long_pools
import observe_ref
import reach_ref
from sparc_gym_amd import _lib
from test_gpu_geometry import MODES, _at_snap, _same
from test_gpu_observe import _small
from test_gpu_snapshot import N, _arrays
from test_gpu_snapshot import _same as _same_arrays
from test_gpu_snapshot import _vec, _warm
from test_gpu_expand import _S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARITY = ("7x7_p8", "w1p4", "w1p12", "w2p7", "w2p15", "7x15_w2p16", "7x7_w4p7", "w4p13")
KEYS = ("dist", "action_dist", "live", "size", "plane")
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257)
N_PARITY = 320
NONE = 255


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _all_same(got, want, case, keys=KEYS):
    for k in keys:
        assert got[k].dtype == np.uint8, (k, case)
        _same(got[k], want[k], k, case)


def _ref_of_records(rec, proc, table, xd, yd):
    """reach_ref on records decoded by tests/observe_ref.py (checked against the oracle elsewhere)."""
    vis, _, pid, loc = observe_ref.decode(rec, table.words, table.pitch, 16, 16)
    return reach_ref.reach(proc, pid, loc[:, 0], loc[:, 1], vis, xd, yd)


# ----------------------------------------------------------------------------- 1. parity with the reference helper
@pytest.mark.parametrize("tb", [True, False])
@pytest.mark.parametrize("name", PARITY)
def test_records_at_step_20_equal_the_breadth_first_search(on_gpu, name, tb):
    """320 envs, 20 steps of geometry_pools.actions under max_steps 24, snapshot, reach: all five
    outputs equal reach_ref on the oracle's state20, pending records included, in both autoreset
    modes; the same without the plane; on 7x7_p8 also with planes padded to 16 x 16."""
    n = N_PARITY
    proc, table, _ = gp.step_pool(name)
    for mode in MODES:
        case = (name, tb, mode)
        v, tr, _ = _at_snap(name, n, tb, mode)
        st = tr["state20"]
        if mode == "none":
            assert (st["pending"] != 0).any()                  # ended episodes stand among the records
        snap = v.snapshot()
        xd, yd = v.x_dim, v.y_dim
        assert (xd, yd) == (table.x_max, table.y_max)
        want = reach_ref.reach(proc, st["pid"], st["x"], st["y"], st["visited"], xd, yd)
        assert (want["dist"] == NONE).any() and (want["live"] != 0).any() and len(np.unique(want["dist"])) >= 14
        out = v.reach(snap, plane=True)
        assert out["plane"].shape == (n, xd, yd) and out["action_dist"].shape == (n, 4)
        _all_same(_host(out), want, case)
        bare = v.reach(snap)
        assert set(bare) == set(KEYS[:4])
        _all_same(_host(bare), want, case, KEYS[:4])
        if name == "7x7_p8":
            v.x_dim = v.y_dim = 16
            big = _host(v.reach(snap, plane=True))
            v.x_dim, v.y_dim = xd, yd
            want16 = reach_ref.reach(proc, st["pid"], st["x"], st["y"], st["visited"], 16, 16)
            assert (want16["plane"][:, xd:] == NONE).all() and (want16["plane"][:, :, yd:] == NONE).all()
            _all_same(big, want16, case + ("16x16",))
        v.core.sync()


# ----------------------------------------------------------------------------- 2. the project's own kernels
@pytest.mark.parametrize("tb", [True, False])
@pytest.mark.parametrize("name", ["7x7_p8", "w2p7", "w4p13"])
def test_reach_agrees_with_observe_and_expand_on_the_same_records(on_gpu, name, tb):
    n = N_PARITY
    proc = gp.step_pool(name)[0]
    for mode in MODES:
        case = (name, tb, mode)
        v, tr, _ = _at_snap(name, n, tb, mode)
        snap = v.snapshot()
        r, ob = v.reach(snap), v.observe(snap)
        live, ad = r["live"].to(torch.int64), r["action_dist"].to(torch.int64)
        assert not (live & ~ob["legal_actions"].to(torch.int64)).any(), case
        bits = ((live[:, None] >> torch.arange(4, device=live.device)) & 1) != 0
        assert torch.equal(bits, ad != NONE), case
        assert bits.any() and not bits.all()
        # the children of expand: exactly one move nearer, wherever the move is live (a pending parent
        # under next_step autoreset has no children of its own: they are the next puzzle's reset state)
        kids = v.reach(v.expand(snap)["children"])["dist"].to(torch.int64).reshape(n, 4)
        own = bits.clone()
        if mode == "next_step":
            own &= ~torch.from_numpy(tr["state20"]["pending"] != 0).cuda()[:, None]
        assert own.sum() > n // 2
        assert torch.equal(kids[own], ad[own] - 1), case
        xy, pid = ob["agent_xy"].cpu().numpy(), ob["puzzle_index"].cpu().numpy()
        on_target = np.array([tuple(proc[int(q)]["target_location"]) == tuple(p) for q, p in zip(pid, xy)])
        assert on_target.any() and np.array_equal(r["dist"].cpu().numpy() == 0, on_target), case
        v.core.sync()


# ----------------------------------------------------------------------------- 3. against dfs
def test_dfs_finds_a_target_exactly_where_reach_says_one_is_left(on_gpu):
    """5 x 5 and 7 x 7 lattices, traceback, max_steps 2000, autoreset none: records after 12 random
    steps, the pending ones dropped; the whole forward subtree of each (dfs, COMPLETE for every root)
    holds a target node exactly where dist is neither 0 (on the target) nor 255 (lost)."""
    from sparc_gym_amd import SPaRCVecEnv
    proc = dfs_ref.pool("A")
    assert {(p["x_size"], p["y_size"]) for p in proc} == {(5, 5), (7, 7)}
    n = 256
    vec = SPaRCVecEnv(n, processed=proc, traceback=True, autoreset="none", observation="compact", max_steps=2000)
    vec.reset(options={"puzzle_index": np.arange(n) % len(proc)})
    vec.rollout(12, None, seed=9)
    snap = vec.snapshot()
    keep = ((snap.records[:, 6] & 4) == 0).nonzero().squeeze(1)   # aux bit 18: the episode has ended
    assert n // 2 < len(keep) < n
    snap = snap.select(keep)
    out = vec.dfs(snap, 1 << 20)
    assert (out["status"] == _lib.DFS_COMPLETE).all()
    targets = out["counts"][:, _lib.DFS_COUNTER_NAMES.index("targets")] > 0
    dist = vec.reach(snap)["dist"]
    assert not (dist == 0).any()                                   # a record on the target is pending
    assert torch.equal(targets, dist != NONE)
    assert targets.any() and not targets.all()
    vec.core.sync()


# ----------------------------------------------------------------------------- 4. long floods
CORRIDOR_X = tuple(range(0, 16, 2))


@functools.lru_cache(maxsize=None)
def _corridor():
    """A 16 x 16 lattice (four words, pitch 16) whose gaps leave one serpentine corridor: the even
    columns whole, joined at alternating ends through the odd ones, from (0, 0) to (14, 0); and one
    more open point, (1, 14), beside the first joint: a short cut of two moves and a dead end."""
    from sparc_gym_amd import synthetic
    from sparc_gym_amd.puzzles import process_puzzles
    base = process_puzzles(synthetic.make_puzzles(1, seed=5, sizes=((7, 7),), full_properties=False))[0]
    gaps = np.ones((16, 16), np.int32)
    acts = []
    for k, x in enumerate(CORRIDOR_X):
        gaps[x, :] = 0
        acts += [1 if k % 2 else 3] * 15
        if x + 2 < 16:
            gaps[x + 1, 0 if k % 2 else 15] = 0
            acts += [0, 0]
    gaps[1, 14] = 0
    path = long_pools.walk((0, 0), acts)
    assert path[-1] == (14, 0) and len(set(path)) == len(path) == 135 and all(gaps[p] == 0 for p in path)
    q = copy.deepcopy(base)
    q["x_size"] = q["y_size"] = 16
    q["obs_array"]["gaps"] = gaps
    q["start_location"], q["target_location"] = [0, 0], [14, 0]
    q["solution_paths"], q["solution_count"] = [[list(pt) for pt in path]], 1
    return [q], acts


def test_a_serpentine_corridor_of_more_than_128_moves(on_gpu):
    from sparc_gym_amd import SPaRCVecEnv
    from sparc_gym_amd.snapshot import Snapshot
    proc, acts = _corridor()
    vec = SPaRCVecEnv(4, processed=proc, traceback=False, autoreset="none", observation="compact", max_steps=2000)
    t = vec.table
    assert (t.words, t.pitch, t.x_max, t.y_max) == (4, 16, 16, 16)
    # the root
    root = vec.roots(np.zeros(1, np.int64))
    got = _host(vec.reach(root, plane=True))
    want = _ref_of_records(root.numpy(), proc, t, 16, 16)
    _all_same(got, want, "root")
    assert got["dist"][0] == 132 and got["size"][0] == 135 and got["plane"][0, 14, 0] == 0    # 134 less the short cut
    assert got["plane"][0, 0, 1] == 131 and got["live"][0] == 0b1000
    # along the corridor: after 1 .. 134 of its moves
    lens = np.array([1, 2, 14, 15, 16, 17, 18, 40, 64, 100, 127, 128, 133, 134], np.int32)
    A = np.repeat(np.array(acts, np.uint8)[:, None], len(lens), axis=1)
    fin = vec.replay(puzzle_indices=np.zeros(len(lens), np.int64), actions=A, lengths=lens)["final"]
    got = _host(vec.reach(fin, plane=True))
    want = _ref_of_records(fin.numpy(), proc, t, 16, 16)
    _all_same(got, want, "corridor")
    assert got["dist"].tolist() == [131, 130, 118, 119, 118, 117, 116, 94, 70, 34, 7, 6, 1, 0]
    # the dead end: round the first joint and into (1, 14) from the far side
    detour = np.array(acts[:18] + [2], np.uint8)[:, None]
    dead = vec.replay(puzzle_indices=np.zeros(1, np.int64), actions=detour)["final"]
    f = dead.fields()
    assert (int(f["x"][0]), int(f["y"][0]), int(f["path_len"][0])) == (1, 14, 20)
    got = _host(vec.reach(dead, plane=True))
    _all_same(got, _ref_of_records(dead.numpy(), proc, t, 16, 16), "dead end")
    assert got["dist"][0] == NONE and got["live"][0] == 0 and got["size"][0] == 136 - 20
    # one corridor point visited behind the agent's back: bit x * 16 + y of the board, (8, 3)
    rec = fin.records.clone()
    b = 8 * 16 + 3
    rec[:, 16 + b // 8] |= 1 << (b % 8)
    got = _host(vec.reach(Snapshot(rec, fin.info), plane=True))
    want = _ref_of_records(rec.cpu().numpy(), proc, t, 16, 16)
    _all_same(got, want, "cut")
    before = lens < 71                                             # (8, 3) is point 71 of the corridor: still ahead
    assert before.sum() == 9 and (got["dist"][before] == NONE).all() and (got["dist"][~before] != NONE).all()
    vec.core.sync()


# ----------------------------------------------------------------------------- 5. sizes and edges
_REF = {}


def _small_ref(S, xd, yd):
    key = (id(S), xd, yd)
    if key not in _REF:
        _REF[key] = _ref_of_records(S["rec"], S["proc"], S["table"], xd, yd)
    return _REF[key]


@pytest.mark.parametrize("M", SIZES)
def test_small_shapes(on_gpu, M):
    """Every M around the wave and workgroup sizes: the rows of a 300-record call, on the 7 x 7 pool
    (49-byte planes: a wave's run ends inside a 16-B piece) and on mixed_5_11 (two words, puzzles
    smaller than the planes)."""
    rows = np.arange(M) * 7 % N
    for pool_name in ("7x7_full", "mixed_5_11"):
        S = _small(pool_name)
        v, t = S["v"], S["table"]
        v.x_dim, v.y_dim = t.x_max, t.y_max
        want = {k: a[rows] for k, a in _small_ref(S, t.x_max, t.y_max).items()}
        whole = _host(v.reach(S["snap"], plane=True))
        got = _host(v.reach(S["snap"].select(rows), plane=True))
        _all_same(got, want, (pool_name, M))
        _all_same({k: a[rows] for k, a in whole.items()}, want, (pool_name, M, "rows of the whole call"))
        v.core.sync()


def _filled(nbytes):
    return torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("M", [65, 257])
def test_each_output_alone_and_nothing_written_outside_it(on_gpu, M):
    """One output per call, the others NULL, each in the middle of a buffer of 0x5A: the bytes equal
    the full call's, the bytes before and after are untouched; at a 16-B aligned start and one byte
    past it (where action_dist and the plane take byte stores)."""
    rows = np.arange(M) * 7 % N
    S = _small("7x7_full")
    v, t = S["v"], S["table"]
    xd, yd = t.x_max, t.y_max
    v.x_dim, v.y_dim = xd, yd
    snap = S["snap"].select(rows)
    rec = snap.records.contiguous()
    full = v.reach(snap, plane=True)
    sizes = {"dist": M, "action_dist": 4 * M, "live": M, "size": M, "plane": M * xd * yd}
    for off in (64, 65):
        for k in KEYS:
            buf = _filled(off + sizes[k] + 64)
            assert buf.data_ptr() % 16 == 0
            v._stream()
            v.core.reach_records_device(snap.info, rec.data_ptr(), M, xd, yd, **{"d_" + k: buf.data_ptr() + off})
            assert torch.equal(buf[off:off + sizes[k]], full[k].reshape(-1)), (k, off, M)
            assert (buf[:off] == 0x5A).all() and (buf[off + sizes[k]:] == 0x5A).all(), (k, off, M)
    v.core.sync()


def test_the_host_form_equals_the_device_form(on_gpu):
    S = _small("mixed_5_11")
    v, t = S["v"], S["table"]
    v.x_dim, v.y_dim = t.x_max, t.y_max
    own = _host(v.reach(S["snap"], plane=True))
    v.core.sync()
    raw = np.empty(S["rec"].size + 1, np.uint8)
    un = raw[1:].reshape(S["rec"].shape)                           # an unaligned copy of the records
    un[:] = S["rec"]
    assert un.ctypes.data % 2 == 1
    h = v.core.reach_records_host(S["snap"].info, un)
    _all_same(h, own, "host")
    h = v.core.reach_records_host(S["snap"].info, un, plane=False)
    assert set(h) == set(KEYS[:4])
    _all_same(h, own, "host, no plane", KEYS[:4])
    h = v.core.reach_records_host(S["snap"].info, un, x_dim=16, y_dim=16)
    assert np.array_equal(h["plane"][:, :t.x_max, :t.y_max], own["plane"]) and (h["plane"][:, t.x_max:] == NONE).all()


@pytest.mark.parametrize("name,tb", [("7x7_full", True), ("mixed_5_11", False)])
def test_bad_records_are_refused_on_the_device(on_gpu, name, tb):
    """Zeroed, puzzle past the table, x or y outside, length 0, trie node past the count, mixed among
    good records in one launch: dist and action_dist 255, live 0, size 0, a plane of 255; the good
    ones exact; sync raises once."""
    from sparc_gym_amd.snapshot import Snapshot
    S = _S(name, tb)
    v = _warm(S)
    snap = v.snapshot()
    P = len(S["proc"])
    good = _host(v.reach(snap, plane=True))
    v.core.sync()
    rec = snap.records.clone()
    damage = {12: ("zero", None), 63: ("pid", P), 64: ("x", 200), 130: ("y", 200), 191: ("len", 0), 192: ("node", None),
              299: ("pid", 2**32 - 1)}
    for k, (what, val) in damage.items():
        if what == "zero":
            rec[k] = 0
        elif what == "pid":
            rec[k, 12:16] = torch.tensor(list(int(val).to_bytes(4, "little")), dtype=torch.uint8, device="cuda")
        elif what == "node":
            rec[k, 4:6] = 0xFF
        else:
            rec[k, {"x": 0, "y": 1, "len": 2}[what]] = val
    out = _host(v.reach(Snapshot(rec, snap.info), plane=True))
    with pytest.raises(ValueError, match="reach"):
        v.core.sync()
    v.core.sync()                                  # the error is reported once
    bad = np.zeros(N, bool)
    bad[list(damage)] = True
    assert (out["dist"][bad] == NONE).all() and (out["action_dist"][bad] == NONE).all() and (out["plane"][bad] == NONE).all()
    assert not out["live"][bad].any() and not out["size"][bad].any()
    for k in KEYS:
        assert np.array_equal(out[k][~bad], good[k][~bad]), k
    again = _host(v.reach(snap, plane=True))       # the next call is clean
    v.core.sync()
    for k in KEYS:
        assert np.array_equal(again[k], good[k]), k


def test_arguments_are_refused_with_a_message(on_gpu):
    S = _S("7x7_full", True)
    v = _warm(S)
    s = v.snapshot()
    X, Y = v.x_dim, v.y_dim
    buf = torch.zeros(N * 256 + 64, dtype=torch.uint8, device="cuda")
    lib, ctx = v.core.lib, v.core.ctx

    def call(rec=s.records.data_ptr(), M=N, **kw):
        a = dict(dist=None, action_dist=None, live=None, size=None, plane=buf.data_ptr(), x_dim=X, y_dim=Y)
        a.update(kw)
        o = _lib.SparcReachOut(**a)
        return lib.sparc_reach_records_device(ctx, ctypes.byref(s.info), rec, M, ctypes.byref(o))

    for kw, what in ((dict(x_dim=X - 1), "x_dim"), (dict(y_dim=Y - 1), "y_dim"), (dict(x_dim=16, y_dim=17), "x_dim"),
                     (dict(x_dim=0), "x_dim"), (dict(M=0), "M must"), (dict(M=2**31), "M must"), (dict(rec=None), "records"),
                     (dict(rec=s.records.data_ptr() + 8), "aligned"), (dict(plane=None), "at least one")):
        assert call(**kw) == -1, kw
        assert what in lib.sparc_last_error(ctx).decode(), (kw, lib.sparc_last_error(ctx))
    assert call() == 0 and call(x_dim=16, y_dim=16) == 0 and call(plane=buf.data_ptr() + 3) == 0
    assert call(plane=None, live=buf.data_ptr(), x_dim=0, y_dim=0) == 0        # the size is read only with a plane
    v.core.sync()
    other = _vec(S, traceback=False)
    with pytest.raises(ValueError, match="traceback|max_steps"):
        other.reach(s)
    with pytest.raises(ValueError, match="traceback"):
        other.core.reach_records_device(s.info, s.records.data_ptr(), N, d_dist=buf.data_ptr())


def test_no_env_is_touched_and_a_caller_stream_gives_the_same_bytes(on_gpu):
    from sparc_gym_amd.snapshot import Snapshot
    from test_gpu_streams import _Gate
    S = _S("mixed_5_11", True)
    v = _warm(S)
    snap = v.snapshot()
    before = _arrays(v)
    own = _host(v.reach(snap, plane=True))
    v.core.sync()
    _same_arrays(_arrays(v), before)
    assert torch.equal(v.snapshot().records, snap.records)
    # a context that was never reset, and never saw a rule table, answers for roots
    w = _vec(S)
    pz = np.arange(N) % len(S["proc"])
    roots = w.roots(pz)
    ro = _host(w.reach(roots, plane=True))
    w.core.sync()
    assert w.core.has_state is False
    _all_same(ro, _ref_of_records(roots.numpy(), S["proc"], S["table"], w.x_dim, w.y_dim), "roots")
    # on a caller's stream: the true records arrive behind a gate on that stream; a launch on any
    # other stream reads the poison (the reset state's records)
    St = torch.cuda.Stream()
    true_r, buf_r = snap.records.clone(), v.roots(np.zeros(N, np.int64)).records.clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(St):
        gate = _Gate(St)
        buf_r.copy_(true_r, non_blocking=True)
        out = v.reach(Snapshot(buf_r, snap.info), plane=True)
        gate.assert_closed("reach")
        assert v._bound_stream == St.cuda_stream
        St.synchronize()
        got = _host(out)
    for k in own:
        assert np.array_equal(got[k], own[k]), k


# ----------------------------------------------------------------------------- 6. search
N_SEARCH = 6


def _pruned_nodes(p):
    """Nodes per depth of the forward-move tree of puzzle p in which a child is entered only if the
    target can still be reached from it (its move is live in the parent): a CPU walk with reach_ref."""
    start = tuple(int(c) for c in p["start_location"])
    target = tuple(int(c) for c in p["target_location"])
    vis = np.zeros((p["x_size"], p["y_size"]), np.int32)
    vis[start] = 1
    nodes = {0: 1}

    def walk(x, y, d):
        if (x, y) == target:
            return
        live = reach_ref.reach_one(p, x, y, vis)[2]
        for a, (dx, dy) in enumerate(reach_ref.DIRS):
            if (live >> a) & 1:
                nodes[d + 1] = nodes.get(d + 1, 0) + 1
                vis[x + dx, y + dy] = 1
                walk(x + dx, y + dy, d + 1)
                vis[x + dx, y + dy] = 0

    walk(*start, 0)
    return [nodes[d] for d in range(len(nodes))]


@pytest.mark.parametrize("tb", [True, False])
def test_pruned_search_finds_the_same_paths_in_fewer_nodes(on_gpu, tb):
    from sparc_gym_amd import SPaRCVecEnv, search
    proc = gp.rule_pool("7x7_p8")[0][:N_SEARCH]
    vec = SPaRCVecEnv(N_SEARCH, processed=proc, traceback=tb, autoreset="none", observation="compact", max_steps=64)
    q = np.arange(N_SEARCH)
    plain = search.solve_by_rules(vec, q)
    again = search.solve_by_rules(vec, q, prune=False)
    pruned = search.solve_by_rules(vec, q, prune=True)
    vec.core.sync()
    assert sum(len(p) for p in plain["paths"]) > N_SEARCH
    assert plain["paths"] == again["paths"] == pruned["paths"]      # the same paths in the same order
    for k in ("bits", "satisfied", "listed"):
        for r in range(N_SEARCH):
            assert np.array_equal(np.asarray(plain[k][r]), np.asarray(again[k][r])), (k, r)
            assert np.array_equal(np.asarray(plain[k][r]), np.asarray(pruned[k][r])), (k, r)
    assert np.array_equal(plain["nodes"], again["nodes"])
    D = pruned["nodes"].shape[1]
    assert D <= plain["nodes"].shape[1]
    assert (pruned["nodes"] <= plain["nodes"][:, :D]).all() and pruned["nodes"].sum() < plain["nodes"].sum()
    for r in range(N_SEARCH):
        want = _pruned_nodes(proc[r])
        assert pruned["nodes"][r, :len(want)].tolist() == want and not pruned["nodes"][r, len(want):].any(), r
    # one level: prune keeps exactly the children whose live bit is set, in the same order
    vec.reset(options={"puzzle_index": q})
    vec.rollout(9, None, seed=4)
    snap = vec.snapshot()
    a, b, c = (search.expand_frontier(vec, snap, **kw) for kw in (dict(), dict(prune=False), dict(prune=True)))
    live = vec.reach(snap)["live"].to(torch.int64)
    for k in ("parent", "action", "reward_code", "flags"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["children"].records, b["children"].records)
    keep = ((live[a["parent"]] >> a["action"]) & 1) != 0
    for k in ("parent", "action", "reward_code", "flags"):
        assert torch.equal(c[k], a[k][keep]), k
    assert torch.equal(c["children"].records, a["children"].records[keep])
    legal = vec.observe(snap)["legal_actions"].to(torch.int64)
    assert torch.equal(torch.bincount(c["parent"], minlength=N_SEARCH),
                       sum(((live & legal) >> k) & 1 for k in range(4)))
    vec.core.sync()
