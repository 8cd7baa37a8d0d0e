"""The pruned depth-first search of state records (k_dfs<.., DfsLiveMoves> through
sparc_dfs_pruned_device, SPaRCVecEnv.dfs(prune=...) and search.solve_dfs_pruned) against the
pruned CPU walker of tests/dfs_prune_ref.py (dfs_ref.Walker with reach_ref's live moves as children),
against the unpruned search on the same roots, and against SPaRCVecEnv.reach.

Pools as tests/test_gpu_dfs.py (tests/test_dfs_prune_ref.py asserts the pruned walks' facts without a
GPU); the helpers of that file are used through the module, the file itself is not touched."""
import numpy as np
import pytest

import dfs_prune_ref
import dfs_ref
import reach_ref
import test_gpu_dfs as base
from dfs_prune_ref import DEADLINE, REACH

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAMES = dfs_ref.COUNTERS
INVALID, COMPLETE, BUDGET, PENDING, OVERFLOW = range(5)
DONE, FOUND, LEAF, STARTED = 1 << 28, 1 << 29, 1 << 30, 1 << 31
MODE = {REACH: "reach", DEADLINE: "deadline"}
TARGET_COLS = [1, 2, 3, 4, 7]                                  # targets, satisfied, listed, both, undecided
counts_of = base.counts_of
reset_roots = base.reset_roots


def make_vec(name, n=None, max_steps=None, **kw):
    from sparc_gym_amd import SPaRCVecEnv
    proc = dfs_ref.pool(name)
    return SPaRCVecEnv(n or len(proc), processed=proc, traceback=True, autoreset="none", observation="compact",
                       max_steps=max_steps or base.MAX_STEPS[name], **kw)


def pruned_walks(name, prune=REACH, max_steps=None):
    kw = dict(searches=True) if name == "A" else {}
    return dfs_prune_ref.complete_walks(name, prune=prune, max_steps=max_steps or base.MAX_STEPS[name], **kw)


def same_answer(cut, full):
    """The five target counters and first, byte for byte, of a pruned and an unpruned complete walk."""
    assert torch.equal(cut["counts"][:, TARGET_COLS], full["counts"][:, TARGET_COLS])
    assert torch.equal(cut["first"].records, full["first"].records) and torch.equal(cut["found"], full["found"])
    assert bool((cut["counts"][:, 0] <= full["counts"][:, 0]).all())


# ----------------------------------------------------------------------------- 1. complete walks
@pytest.mark.parametrize("prune,max_steps", [(REACH, None), (DEADLINE, None), (DEADLINE, 9), (DEADLINE, 14)])
def test_complete_walks_one_word(on_gpu, prune, max_steps):
    ws = pruned_walks("A", prune, max_steps)
    for kw in ({}, dict(rule_table_entries=1)):               # the table-only and the generic one-word kernel
        vec = make_vec("A", max_steps=max_steps, **kw)
        assert vec.table.words == 1
        roots = reset_roots(vec)
        out = vec.dfs(roots, 1 << 20, prune=MODE[prune])
        base.check_complete(out, roots, ws)
        c = out["counts"].cpu().numpy()
        assert (c[:, 5] == (c[:, 0] == 0)).all()              # a dead end only at a root that is cut off
        if prune == DEADLINE:
            assert not c[:, 6].any()
        same_answer(out, vec.dfs(roots, 1 << 20))
        mode = (out["state"].cpu().numpy().astype(np.int64) >> 12) & 3
        assert (mode == prune).all()
        vec.core.sync()
    if max_steps == 9:
        assert any(w.counts["nodes"] == 0 for w in ws)        # a start the limit cuts off: one root dead end
    if prune == REACH:                                        # True is "reach"; and the host-pointer form
        again = vec.dfs(roots, 1 << 20, prune=True)
        assert torch.equal(again["counts"], out["counts"]) and torch.equal(again["state"], out["state"])
        host = vec.core.dfs_host(roots.info, roots.numpy(), 1 << 20, prune=REACH)
        assert np.array_equal(host["counts"].astype(np.int64), np.stack([counts_of(w) for w in ws]))
        assert (host["status"] == COMPLETE).all() and np.array_equal(host["cursor"], roots.numpy())
        vec.core.sync()


@pytest.mark.parametrize("prune,max_steps", [(REACH, None), (DEADLINE, None), (DEADLINE, 16)])
def test_complete_walks_two_words(on_gpu, prune, max_steps):
    ws = pruned_walks("B", REACH if max_steps is None else prune, max_steps)   # no limit in reach: the same walk
    vec = make_vec("B", max_steps=max_steps)
    assert vec.table.words == 2
    roots = reset_roots(vec)
    out = vec.dfs(roots, 1 << 20, prune=MODE[prune])
    base.check_complete(out, roots, ws)
    c = out["counts"].cpu().numpy()
    assert (c[:, 5] == (c[:, 0] == 0)).all() and (prune == REACH or not c[:, 6].any())
    same_answer(out, vec.dfs(roots, 1 << 20))
    vec.core.sync()


def pool_c_snapshot(vec):
    """Pool C's 16 roots as test_gpu_dfs.test_four_words writes them (records by hand, tests/record_path.py)."""
    from record_path import encode
    from sparc_gym_amd.puzzles import build_trie
    from sparc_gym_amd.snapshot import Snapshot
    from test_dfs_ref import pool_c_roots
    rc = pool_c_roots()
    info = vec.core.snapshot_info()
    rows = []
    for q, pre in rc:
        p = vec.puzzles[q]
        nodes, valid = build_trie(tuple(int(v) for v in p["start_location"]), p["solution_paths"][:p["solution_count"]])
        node = 0
        for a in pre:
            node = nodes[node][a]
        assert valid and node != 0xFFFF
        rows.append(encode(info, q, dfs_ref.points_of(p, pre), step=len(pre), aux=node | (nodes[node][5] << 19)))
    return rc, Snapshot(torch.from_numpy(np.stack(rows)).cuda(), info)


@pytest.mark.parametrize("prune", [REACH, DEADLINE])
def test_four_words(on_gpu, prune):
    """Budget 3000 and one continuation, as the unpruned test: status, counters, cursor and first after
    each call equal the pruned walker's; where both searches complete, the answer is the unpruned one's."""
    vec = make_vec("C", n=1)
    assert vec.table.words == 4
    rc, roots = pool_c_snapshot(vec)
    walkers = [dfs_prune_ref.PrunedWalker(vec.puzzles[q], pre, prune=prune, root_step=len(pre),
                                          max_steps=base.MAX_STEPS["C"]) for q, pre in rc]
    out = vec.dfs(roots, 3000, prune=MODE[prune])
    full = vec.dfs(roots, 3000)
    for call in range(2):
        for w in walkers:
            w.run(3000)
        assert out["status"].cpu().tolist() == [COMPLETE if w.complete else BUDGET for w in walkers]
        assert np.array_equal(out["counts"].cpu().numpy(), np.stack([counts_of(w) for w in walkers]))
        assert out["cursor"].moves() == [w.path for w in walkers]
        assert out["first"].moves() == [w.first or [] for w in walkers]
        if call == 0:
            out = vec.dfs(out["cursor"], 3000, state=out["state"], counts=out["counts"], first=out["first"],
                          prune=MODE[prune])
            full = vec.dfs(full["cursor"], 3000, state=full["state"], counts=full["counts"], first=full["first"])
    both = (out["done"] & full["done"]).nonzero().squeeze(1)
    assert len(both) >= 12
    assert torch.equal(out["counts"][both][:, TARGET_COLS], full["counts"][both][:, TARGET_COLS])
    assert torch.equal(out["first"].records[both], full["first"].records[both])
    assert bool((out["counts"][both, 0] < full["counts"][both, 0]).any())
    c = out["counts"].cpu().numpy()
    assert (c[:, 5] == (c[:, 0] == 0)).all() and (c[:, 0] == 0).any()         # some prefixes are walled off
    done = out["done"].nonzero().squeeze(1)
    assert torch.equal(out["cursor"].records[done], roots.records[done])
    vec.core.sync()


# ----------------------------------------------------------------------------- 2. budget and resume
def unpruned_move_left(p, acts, max_steps):
    """Standing on the node ``acts``, does the way back up to the start pass an untried forward move
    of the UNPRUNED tree?  (CPU)"""
    u = dfs_ref.Walker(p, list(acts), max_steps=max_steps)
    u.root_len, u.leaf = 1, True
    while len(u.pts) > 1:
        u._undo()
        if u._forward(u.next):
            return True
    return False


@pytest.mark.parametrize("budget", [1, 7, 1000])
@pytest.mark.parametrize("name", ["A", "B"])
def test_budget_and_resume(on_gpu, name, budget):
    """As test_gpu_dfs.test_budget_and_resume, on sparc_dfs_pruned_device with prune = 1.  The call that
    enters a walk's last node must report COMPLETE: every sibling its look-ahead passes on the way
    back up is dead, although (asserted on the CPU) the unpruned tree has forward moves there."""
    ws = pruned_walks(name)
    proc = dfs_ref.pool(name)
    assert any(unpruned_move_left(p, w.trace[-1][1], base.MAX_STEPS[name]) for p, w in zip(proc, ws))
    vec = make_vec(name)
    vec._load_rules()
    vec._stream()
    roots = reset_roots(vec)
    M, rb, W = len(roots), roots.info.record_bytes, vec.table.words
    totals = np.array([w.counts["nodes"] for w in ws])
    calls = int(-(-totals.max() // budget))
    dev = "cuda"
    cur = roots.records.clone()
    state = torch.zeros(M, dtype=torch.int32, device=dev)
    counts = torch.zeros((M, 8), dtype=torch.int64, device=dev)
    first = torch.zeros((M, rb), dtype=torch.uint8, device=dev)
    status = torch.zeros(M, dtype=torch.uint8, device=dev)
    K = calls + 1                                                             # one more call on the finished state
    h_counts = torch.zeros((K, M, 8), dtype=torch.int64, device=dev)
    h_state = torch.zeros((K, M), dtype=torch.int32, device=dev)
    h_status = torch.zeros((K, M), dtype=torch.uint8, device=dev)
    h_cur = torch.zeros((K, M, rb), dtype=torch.uint8, device=dev)
    for k in range(K):
        vec.core.dfs_device(roots.info, cur.data_ptr(), M, budget, state.data_ptr(), status.data_ptr(),
                            counts.data_ptr(), cur.data_ptr(), first.data_ptr(), prune=REACH)
        h_counts[k].copy_(counts), h_state[k].copy_(state), h_status[k].copy_(status), h_cur[k].copy_(cur)
    vec.core.sync()
    width = max(len(t[1]) for w in ws for t in w.trace)
    for j, w in enumerate(ws):
        n = np.minimum(np.arange(1, K + 1) * budget, totals[j])              # nodes after each call
        cum = np.array([t[0] for t in w.trace], np.int64)
        assert np.array_equal(h_counts[:, j].cpu().numpy(), cum[n]), j
        open_ = np.arange(1, K + 1) * budget < totals[j]
        st, sw = h_status[:, j].cpu().numpy(), h_state[:, j].cpu().numpy().astype(np.int64)
        assert np.array_equal(st, np.where(open_, BUDGET, COMPLETE)), j
        assert np.array_equal((sw & DONE) != 0, ~open_) and ((sw & 0xFF) == 1).all() and not (sw & LEAF).any()
        assert (((sw >> 12) & 3) == REACH).all()
        ref = np.full((len(w.trace), width), 255, np.uint8)
        for i, t in enumerate(w.trace):
            ref[i, :len(t[1])] = np.frombuffer(t[1], np.uint8)
        got = base._moves_padded(h_cur[:, j], W, width).cpu().numpy()
        assert np.array_equal(got[open_], ref[n[open_]]), j                   # the walker's current path
        assert torch.equal(h_cur[~torch.from_numpy(open_).to(dev), j],
                           roots.records[j].expand(int((~open_).sum()), rb)), j
    assert torch.equal(h_counts[-1], h_counts[-2])                            # the extra call added nothing
    from sparc_gym_amd.snapshot import Snapshot
    fm = Snapshot(first, roots.info).moves()
    for j, w in enumerate(ws):
        assert fm[j] == (w.first or []) and (w.first is not None or not first[j].any())


# ----------------------------------------------------------------------------- 3. agreement with reach
REACH_SEED, REACH_M, REACH_L = 3, 64, 16


def random_paths(proc, M, L, seed):
    """M random self-avoiding forward paths that stop short of the target (CPU): actions [L, M] (255
    past the end), lengths [M], and per state (t, j) the puzzle, the agent and the visited plane."""
    rng = np.random.default_rng(seed)
    acts, lengths, states = np.full((L, M), 255, np.uint8), np.zeros(M, np.int32), []
    for j in range(M):
        p = proc[j % len(proc)]
        w = dfs_ref.Walker(p)
        for t in range(int(rng.integers(1, L + 1))):
            x, y = w.pts[-1]
            f = [a for a in w._forward() if (x + dfs_ref.DIRS[a][0], y + dfs_ref.DIRS[a][1]) != w.target]
            if not f:
                break
            a = int(f[int(rng.integers(len(f)))])
            pt = (x + dfs_ref.DIRS[a][0], y + dfs_ref.DIRS[a][1])
            w.pts.append(pt), w.acts.append(a), w.on.add(pt)
            acts[t, j] = a
            vis = np.zeros((w.X, w.Y), np.uint8)
            for q in w.pts:
                vis[q] = 1
            states.append((t, j, p, pt, vis))
        lengths[j] = len(w.acts)
    return acts, lengths, states


def reach_sample():
    proc = dfs_ref.pool("A")
    acts, lengths, states = random_paths(proc, REACH_M, REACH_L, REACH_SEED)
    live = np.array([reach_ref.reach_one(p, *pt, vis)[2] for _, _, p, pt, vis in states])
    legal = np.array([reach_ref.forward_legal(p, *pt, vis) for _, _, p, pt, vis in states])
    return acts, lengths, states, live, legal


def test_first_entry_agrees_with_reach(on_gpu):
    from sparc_gym_amd.snapshot import Snapshot
    acts, lengths, states, live, legal = reach_sample()
    low = lambda m: m & -m                                                    # noqa: E731
    assert len(states) >= 200 and (live == 0).any() and (live != 0).any()
    assert ((live != 0) & (low(legal) != low(live))).any()                    # the lowest legal move is dead there
    assert ((live & ~legal) == 0).all()
    vec = make_vec("A")
    P, M = vec.num_puzzles, REACH_M
    rep = vec.replay(puzzle_indices=np.arange(M) % P, actions=acts, lengths=lengths, states=True, final=False)
    rows = torch.tensor([t * M + j for t, j, *_ in states], device="cuda")
    snap = rep["states"].select(rows)
    assert np.array_equal(vec.reach(snap)["live"].cpu().numpy(), live)
    kids = vec.expand(snap)["children"].records.reshape(len(snap), 4, -1)
    out = vec.dfs(snap, 1, prune=True)
    status, c = out["status"].cpu().numpy(), out["counts"].cpu().numpy()
    cur = out["cursor"].records
    for i in range(len(snap)):
        if live[i] == 0:                                                      # walled off: one dead end, no node
            assert status[i] == COMPLETE and c[i].tolist() == [0, 0, 0, 0, 0, 1, 0, 0], i
            assert torch.equal(cur[i], snap.records[i]), i
        else:
            a = int(low(int(live[i]))).bit_length() - 1
            assert c[i, 0] == 1 and not c[i, 5] and not c[i, 6], i
            if status[i] == BUDGET:
                assert torch.equal(cur[i], kids[i, a]), i                     # expand's child, byte for byte
            else:                                                             # that child was the whole tree
                assert status[i] == COMPLETE and c[i, 1] == 1 and torch.equal(cur[i], snap.records[i]), i
                assert bin(int(live[i])).count("1") == 1
    assert (status == BUDGET).sum() >= len(snap) // 4
    assert isinstance(out["cursor"], Snapshot)
    vec.core.sync()


# ----------------------------------------------------------------------------- 4. ragged waves
def ragged_kinds(vec):
    """Six kinds of record of pool A (puzzle 7 is a 7 x 7, puzzle 0 a 5 x 5), with the state word each
    starts from: a big start, a walled-off root, a pending root, a finished walk's word, a small start
    and a node inside the big tree."""
    from sparc_gym_amd.snapshot import Snapshot
    q = 7
    proc = dfs_ref.pool("A")
    assert (proc[q]["x_size"], proc[0]["x_size"]) == (7, 5)
    w = dfs_ref.complete_walks("A", searches=True, max_steps=base.MAX_STEPS["A"])[q]
    target = next(iter(w.leaves))

    def walled(acts):
        pts = dfs_ref.points_of(proc[q], acts)
        vis = np.zeros((7, 7), np.uint8)
        for pt in pts:
            vis[pt] = 1
        return (reach_ref.reach_one(proc[q], *pts[-1], vis)[2] == 0 and
                reach_ref.forward_legal(proc[q], *pts[-1], vis) != 0 and pts[-1] != w.target)
    off = next(list(t[1]) for t in w.trace[1:] if walled(t[1]))               # forward moves, but none live
    inside = list(pruned_walks("A")[q].trace[2][1])                           # a node of the pruned tree, 2 deep
    assert dfs_prune_ref.walk(proc[q], inside, max_steps=base.MAX_STEPS["A"], root_step=2).counts["nodes"] > 300
    snaps = [base.step_to(vec, q, []), base.step_to(vec, q, off), base.step_to(vec, q, target),
             base.step_to(vec, q, []), base.step_to(vec, 0, []), base.step_to(vec, q, inside)]
    words = np.array([0, 0, 0, DONE | STARTED | 1, 0, 0], np.uint32).view(np.int32)
    return Snapshot.cat(snaps), words


@pytest.mark.parametrize("M", [1, 65, 257])
def test_ragged_waves(on_gpu, M):
    """Roots of very different subtree sizes in one wave, with lanes that never walk (pending, done
    word, damaged, walled off) and lanes that look ahead after the budget while others still flood:
    every valid record gets what it gets alone, over a budgeted call and its continuation."""
    from sparc_gym_amd.snapshot import Snapshot
    vec = make_vec("A")
    kinds, words = ragged_kinds(vec)
    K = len(kinds)
    kind = np.arange(M) % K
    bad = M // 2 if M > 1 else None
    rec = kinds.records[torch.from_numpy(kind).cuda()].clone()
    if bad is not None:
        rec[bad] = 0                                                          # path length 0: refused
    state0 = torch.from_numpy(words[kind]).cuda()

    def run(records, state, budget2):
        snap = Snapshot(records, kinds.info)
        a = vec.dfs(snap, 300, state=state.clone(), prune=True)
        keep = {k: (a[k].records if isinstance(a[k], Snapshot) else a[k]).clone() for k in
                ("status", "counts", "state", "cursor", "first")}
        b = vec.dfs(a["cursor"], budget2, state=a["state"], counts=a["counts"], first=a["first"], prune=True)
        return keep, {k: (b[k].records if isinstance(b[k], Snapshot) else b[k]) for k in keep}

    alone = []
    for k in range(K):
        alone.append(run(kinds.records[k:k + 1].clone(), torch.from_numpy(words[k:k + 1]).cuda(), 1 << 20))
    vec.core.sync()
    assert [int(a[0]["status"][0]) for a in alone] == [BUDGET, COMPLETE, PENDING, COMPLETE, COMPLETE, BUDGET]
    assert alone[1][0]["counts"][0].tolist() == [0, 0, 0, 0, 0, 1, 0, 0] and not alone[3][0]["counts"].any()
    first, second = run(rec, state0, 1 << 20)
    if bad is not None:
        with pytest.raises(ValueError, match="record"):
            vec.core.sync()
    vec.core.sync()
    for got, which in ((first, 0), (second, 1)):
        for j in range(M):
            if j == bad:
                assert int(got["status"][j]) == (INVALID if which == 0 else COMPLETE)
                assert not got["cursor"][j].any() and not got["counts"][j].any()
                assert int(got["state"][j]) & DONE
                continue
            want = alone[kind[j]][which]
            for k in want:
                assert torch.equal(got[k][j], want[k][0]), (which, j, k)
    ws = pruned_walks("A")
    big = second["counts"][0].cpu().numpy()
    assert np.array_equal(big, counts_of(ws[7])) and int(second["status"][0]) == COMPLETE


# ----------------------------------------------------------------------------- 5. the mode in the state word
def test_mode_in_the_state_word(on_gpu):
    from sparc_gym_amd.snapshot import Snapshot
    vec = make_vec("A")
    roots = reset_roots(vec)
    R = len(roots)
    outs = {m: vec.dfs(roots, 5, prune=m) for m in (False, "reach", "deadline")}
    vec.core.sync()
    for m, o in outs.items():
        assert (o["status"] == BUDGET).all()
        assert (((o["state"].to(torch.int64) >> 12) & 3) == {False: 0, "reach": 1, "deadline": 3}[m]).all()
    order = (False, "reach", "deadline")
    cur = Snapshot.cat([outs[m]["cursor"] for m in order])
    state = torch.cat([outs[m]["state"] for m in order])
    counts = torch.cat([outs[m]["counts"] for m in order])
    first = torch.cat([outs[m]["first"].records for m in order])
    for k, m in enumerate(order):
        mine = slice(k * R, (k + 1) * R)
        c0 = counts.clone()
        got = vec.dfs(cur, 1 << 20, state=state.clone(), counts=c0, first=first.clone(), prune=m)
        with pytest.raises(ValueError, match="record"):
            vec.core.sync()
        vec.core.sync()
        other = torch.ones(3 * R, dtype=torch.bool, device="cuda")
        other[mine] = False
        assert (got["status"][other] == INVALID).all() and (got["status"][mine] == COMPLETE).all()
        assert not got["cursor"].records[other].any() and got["done"].all()
        assert torch.equal(got["counts"][other], counts[other])                # untouched
        alone = vec.dfs(outs[m]["cursor"], 1 << 20, state=outs[m]["state"].clone(), counts=outs[m]["counts"].clone(),
                        first=outs[m]["first"].records.clone(), prune=m)
        for key in ("status", "counts", "state"):
            assert torch.equal(got[key][mine], alone[key]), (m, key)
        assert torch.equal(got["cursor"].records[mine], roots.records)
        assert torch.equal(got["first"].records[mine], alone["first"].records)
        vec.core.sync()
    # a word written by sparc_dfs_device itself continues under prune = 0 of the new entry
    rb = roots.info.record_bytes
    cur = roots.records.clone()
    state = torch.zeros(R, dtype=torch.int32, device="cuda")
    status = torch.zeros(R, dtype=torch.uint8, device="cuda")
    counts = torch.zeros((R, 8), dtype=torch.int64, device="cuda")
    first = torch.zeros((R, rb), dtype=torch.uint8, device="cuda")
    vec.core.dfs_device(roots.info, cur.data_ptr(), R, 5, state.data_ptr(), status.data_ptr(), counts.data_ptr(),
                        cur.data_ptr(), first.data_ptr())
    assert torch.equal(state, outs[False]["state"]) and torch.equal(cur, outs[False]["cursor"].records)
    out = vec.dfs(Snapshot(cur, roots.info), 1 << 20, state=state, counts=counts, first=first, prune=False)
    base.check_complete(out, roots, dfs_ref.complete_walks("A", searches=True, max_steps=base.MAX_STEPS["A"]))
    vec.core.sync()


# ----------------------------------------------------------------------------- 6. undecided leaves and OVERFLOW
def test_undecided_overflow_resumes_at_the_leaf(on_gpu):
    """The capped pool of test_gpu_dfs (node cap 1, no region-code table: every exact-fit search is
    undecided) under pruning: the same undecided leaves as the unpruned walk, and a walk that
    overflowed resumes at its leaf without counting the node twice."""
    vec = make_vec("A", fit_cap=1, rule_table_entries=1)
    vec._load_rules()
    vec.core.set_variant(vec.core.VARIANT_HOST_FITS, 1)
    roots = reset_roots(vec)
    ws = [dfs_prune_ref.walk(p, prune=REACH, max_steps=base.MAX_STEPS["A"], searches=True, undecided=base._searched)
          for p in dfs_ref.pool("A")]
    assert [w.counts["undecided"] for w in ws] == [0, 0, 0, 0, 110, 0, 5, 34]   # as unpruned
    want = np.stack([counts_of(w) for w in ws])
    leaves = sorted((j, a) for j, w in enumerate(ws) for a, leaf in w.leaves.items() if leaf["searched"])
    out = vec.dfs(roots, 1 << 20, undecided=16, prune=True)
    assert (out["status"].cpu().numpy() == OVERFLOW).sum() >= 2 and out["undecided_total"] > 16
    seen, calls = [], 1
    while True:
        st = out["state"].cpu().numpy().astype(np.int64)
        assert np.array_equal((st & LEAF) != 0, out["status"].cpu().numpy() == OVERFLOW)
        assert len(out["undecided"]) == min(out["undecided_total"], 16)
        seen += list(zip(out["undecided_root"].cpu().tolist(), map(tuple, out["undecided"].moves())))
        if bool(out["done"].all()):
            break
        out = vec.dfs(out["cursor"], 1 << 20, state=out["state"], counts=out["counts"], first=out["first"],
                      undecided=16, prune=True)
        calls += 1
    assert calls >= -(-149 // 16)
    assert np.array_equal(out["counts"].cpu().numpy(), want)                  # nothing lost, nothing twice
    assert sorted(seen) == leaves
    assert torch.equal(out["cursor"].records, roots.records)
    full = vec.dfs(roots, 1 << 20, undecided=1024)                            # the unpruned walk's undecided leaves
    assert sorted(zip(full["undecided_root"].cpu().tolist(), map(tuple, full["undecided"].moves()))) == leaves
    assert torch.equal(full["counts"][:, TARGET_COLS], out["counts"][:, TARGET_COLS])
    vec.core.sync()


# ----------------------------------------------------------------------------- 7. geometry
GEOM_MAX_STEPS, GEOM_DEPTH, GEOM_CUT, GEOM_ROOTS = 64, 9, 5, 6


def geometry_roots(name):
    """(puzzle, actions from the start) of up to six roots of the class's rule pool: the first stored
    solution of the first puzzles that have one of 6 .. 60 moves, cut 5 moves before its end.  A
    complete walk from the start of a 15 x 5 or 15 x 9 lattice is far too long, so the roots stand a
    few moves above the leaves, and (see the test) step so late that the tree ends 9 steps below."""
    import geometry_pools as gp
    from record_path import DIRS
    proc = gp.rule_pool(name)[0]
    out = []
    for q, p in enumerate(proc):
        if p["solution_count"] < 1:
            continue
        sp = p["solution_paths"][0]
        sol = [DIRS.index((int(b[0]) - int(a[0]), int(b[1]) - int(a[1]))) for a, b in zip(sp[:-1], sp[1:])]
        if GEOM_CUT < len(sol) <= GEOM_MAX_STEPS - GEOM_DEPTH + GEOM_CUT:
            out.append((q, sol[:len(sol) - GEOM_CUT]))
        if len(out) == GEOM_ROOTS:
            break
    return out


@pytest.mark.parametrize("name", ["w1p4", "w2p5", "w4p9"])
def test_geometry(on_gpu, name):
    """The one-word board that fills all 64 bits and a two- and a four-word class whose pitch equals
    y_max (the flood's column masks matter there).  Each root takes idle steps first (replay's
    no-move action 255) so that it stands at step max_steps - 9: the unpruned-by-time tree below it
    is at most 9 deep, the target 5 moves away."""
    import geometry_pools as gp
    from sparc_gym_amd import SPaRCVecEnv
    proc, table = gp.rule_pool(name)[:2]
    if name != "w1p4":
        assert table.pitch == table.y_max
    roots = geometry_roots(name)
    assert len(roots) >= 4
    vec = SPaRCVecEnv(len(roots), processed=proc, table=table, traceback=True, max_steps=GEOM_MAX_STEPS,
                      autoreset="none", observation="compact")
    step0 = GEOM_MAX_STEPS - GEOM_DEPTH
    acts = np.full((step0, len(roots)), 255, np.uint8)
    for j, (q, pre) in enumerate(roots):
        acts[step0 - len(pre):, j] = pre
    snap = vec.replay(puzzle_indices=np.array([q for q, _ in roots]), actions=acts)["final"]
    f = snap.fields()
    assert (f["step"] == step0).all() and f["path_len"].cpu().tolist() == [len(pre) + 1 for _, pre in roots]
    full = vec.dfs(snap, 1 << 20)
    for prune in (REACH, DEADLINE):
        ws = [dfs_prune_ref.walk(proc[q], pre, prune=prune, root_step=step0, max_steps=GEOM_MAX_STEPS)
              for q, pre in roots]
        assert sum(w.counts["targets"] for w in ws) >= len(roots)
        out = vec.dfs(snap, 1 << 20, prune=MODE[prune])
        assert (out["status"] == COMPLETE).all() and torch.equal(out["cursor"].records, snap.records)
        assert np.array_equal(out["counts"].cpu().numpy(), np.stack([counts_of(w) for w in ws])), (name, prune)
        assert out["first"].moves() == [w.first or [] for w in ws]
        same_answer(out, full)
        for budget in (3,):                                                   # and under a budget
            part = vec.dfs(snap, budget, prune=MODE[prune])
            while not bool(part["done"].all()):
                part = vec.dfs(part["cursor"], budget, state=part["state"], counts=part["counts"],
                               first=part["first"], prune=MODE[prune])
            assert torch.equal(part["counts"], out["counts"])
            assert torch.equal(part["first"].records, out["first"].records)
    vec.core.sync()


# ----------------------------------------------------------------------------- 8. solve_dfs
@pytest.mark.parametrize("budget", [7, 4096])
@pytest.mark.parametrize("min_roots", [1, 64])
@pytest.mark.parametrize("name", ["A", "B"])
def test_solve_dfs(on_gpu, name, min_roots, budget):
    from sparc_gym_amd import search
    ws = pruned_walks(name)
    vec = make_vec(name)
    res = search.solve_dfs_pruned(vec, np.arange(vec.num_puzzles), min_roots=min_roots, budget=budget)
    vec.core.sync()
    for k in NAMES:
        assert res[k].dtype == np.int64 and np.array_equal(res[k], [w.counts[k] for w in ws]), k
    assert res["complete"].all() and not res["dead_ends"].any()
    full = search.solve_dfs(vec, np.arange(vec.num_puzzles), min_roots=min_roots, budget=4096)
    assert res["solution"] == full["solution"] == [w.first for w in ws]
    for k in ("targets", "satisfied", "listed", "both", "undecided"):
        assert np.array_equal(res[k], full[k]), k
    assert (res["nodes"] < full["nodes"]).all()
    vec.core.sync()


def test_solve_dfs_walled_off_start(on_gpu):
    """A start whose target is cut off by gaps: one dead end, no node, no split."""
    import copy
    from sparc_gym_amd import SPaRCVecEnv, search
    proc = copy.deepcopy(dfs_ref.pool("A")[:2])
    p = proc[1]
    tx, ty = (int(v) for v in p["target_location"])
    gaps = np.array(p["obs_array"]["gaps"], copy=True)
    for dx, dy in reach_ref.DIRS:
        if 0 <= tx + dx < p["x_size"] and 0 <= ty + dy < p["y_size"]:
            gaps[tx + dx, ty + dy] = 1
    p["obs_array"]["gaps"] = gaps
    w = [dfs_prune_ref.walk(q, max_steps=64) for q in proc]
    assert counts_of(w[1]).tolist() == [0, 0, 0, 0, 0, 1, 0, 0] and w[0].counts["nodes"] > 0
    vec = SPaRCVecEnv(2, processed=proc, traceback=True, autoreset="none", observation="compact", max_steps=64)
    for min_roots in (1, 64):
        res = search.solve_dfs_pruned(vec, np.arange(2), min_roots=min_roots, budget=64, prune="reach")
        for k in NAMES:
            assert np.array_equal(res[k], [x.counts[k] for x in w]), (min_roots, k)
        assert res["complete"].all() and res["solution"][1] is None
    vec.core.sync()


# ----------------------------------------------------------------------------- 9. refused arguments
def test_arguments_are_checked_before_any_launch(on_gpu):
    from sparc_gym_amd import SPaRCVecEnv, search
    proc = dfs_ref.pool("A")
    kw = dict(processed=proc, autoreset="none", observation="compact", max_steps=64)
    flat = SPaRCVecEnv(8, traceback=False, **kw)
    with pytest.raises(ValueError, match="traceback"):
        flat.dfs(reset_roots(flat), 10, prune=True)
    flat._load_rules()
    s = reset_roots(flat)
    z = torch.zeros(8 * 64 + 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="needs a traceback context"):       # the library's own check
        flat.core.dfs_device(s.info, s.records.data_ptr(), 8, 10, z.data_ptr(), z.data_ptr(), z.data_ptr(),
                             z.data_ptr(), prune=REACH)
    vec = SPaRCVecEnv(8, traceback=True, **kw)
    s = reset_roots(vec)
    rb = s.info.record_bytes
    state = torch.zeros(8, dtype=torch.int32, device="cuda")
    status = torch.full((8,), 99, dtype=torch.uint8, device="cuda")
    counts = torch.zeros((8, 8), dtype=torch.int64, device="cuda")
    cur = torch.zeros((8, rb), dtype=torch.uint8, device="cuda")
    args = dict(info=s.info, d_records=s.records.data_ptr(), M=8, budget=10, d_state=state.data_ptr(),
                d_status=status.data_ptr(), d_counts=counts.data_ptr(), d_cursor=cur.data_ptr())
    vec._load_rules()
    for bad in (2, 4, -1):
        with pytest.raises(ValueError, match="prune must be"):
            vec.core.dfs_device(**args, prune=bad)
        with pytest.raises(ValueError, match="prune must be"):
            vec.core.dfs_host(s.info, s.numpy(), 10, prune=bad)
    with pytest.raises(ValueError, match="16-B aligned"):                      # the other checks still hold
        vec.core.dfs_device(**{**args, "d_cursor": cur.data_ptr() + 4}, prune=REACH)
    for bad in (2, "both", None, 3, 1.5):
        with pytest.raises(ValueError, match="prune must be"):
            vec.dfs(s, 10, prune=bad)
    with pytest.raises(ValueError, match="reach only"):
        search.solve_dfs_pruned(vec, np.arange(8), prune="deadline")
    vec.core.sync()
    assert (status == 99).all() and not counts.any() and not state.any()      # nothing was launched
