"""The depth-first subtree search of state records (k_dfs through sparc_dfs_device, SPaRCVecEnv.dfs
and search.solve_dfs) against the CPU walker of tests/dfs_ref.py: the same pre-order walk of the
forward-move tree in pure Python, audited by oracle/rules_ref.py.

Pools (tests/test_dfs_ref.py asserts their facts without a GPU): A 5 x 5 and 7 x 7 lattices, one
word, 613 target paths, 149 of them with an exact-fit search; B 9 x 9, two words, 17,876 target
paths over 385,724 nodes; C two-walled 15 x 15, four words, roots deep inside a solution.
"""
import numpy as np
import pytest

import dfs_ref
from test_dfs_ref import pool_c_roots

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MAX_STEPS = {"A": 64, "B": 128, "C": 256}
NAMES = dfs_ref.COUNTERS
INVALID, COMPLETE, BUDGET, PENDING, OVERFLOW = range(5)
DONE, FOUND, LEAF = 1 << 28, 1 << 29, 1 << 30


def make_vec(name, n=None, **kw):
    from sparc_gym_amd import SPaRCVecEnv
    proc = dfs_ref.pool(name)
    return SPaRCVecEnv(n or len(proc), processed=proc, traceback=True, autoreset="none", observation="compact",
                       max_steps=MAX_STEPS[name], **kw)


def reset_roots(vec, R=None):
    R = vec.num_puzzles if R is None else R
    vec.reset(options={"puzzle_index": np.arange(vec.num_envs) % vec.num_puzzles})
    return vec.snapshot(envs=np.arange(R))


def counts_of(w):
    return np.array([w.counts[k] for k in NAMES], np.int64)


def step_to(vec, q, actions, idle=0):
    """The record of puzzle q after ``idle`` no-move steps (action 255) and then ``actions``, walked by env 0."""
    vec.reset(options={"puzzle_index": np.full(vec.num_envs, q)})
    for a in [255] * idle + list(actions):
        vec.step(torch.full((vec.num_envs,), a, dtype=torch.int64, device="cuda"))
    return vec.snapshot(envs=[0])


@pytest.fixture(scope="module")
def walks():
    """The CPU side, computed once: the traced complete walks of pools A and B."""
    return {"A": dfs_ref.complete_walks("A", searches=True, max_steps=MAX_STEPS["A"]),
            "B": dfs_ref.complete_walks("B", max_steps=MAX_STEPS["B"])}


def check_complete(out, roots, ws):
    assert (out["status"].cpu().numpy() == COMPLETE).all() and bool(out["done"].all())
    assert np.array_equal(out["counts"].cpu().numpy(), np.stack([counts_of(w) for w in ws]))
    firsts, found = out["first"].moves(), out["found"].cpu().numpy()
    for j, w in enumerate(ws):
        assert found[j] == (w.first is not None)
        if w.first is None:
            assert not out["first"].records[j].any()
        else:
            assert firsts[j] == w.first
    assert torch.equal(out["cursor"].records, roots.records)                 # the root again, byte for byte


# ----------------------------------------------------------------------------- 1. complete walks
@pytest.mark.parametrize("name", ["A", "B"])
def test_complete_walks(on_gpu, walks, name):
    vec = make_vec(name)
    assert vec.table.words == {"A": 1, "B": 2}[name]
    roots = reset_roots(vec)
    out = vec.dfs(roots, 1 << 20)
    check_complete(out, roots, walks[name])
    assert out["counts"].dtype == torch.int64 and out["status"].dtype == torch.uint8
    assert out["state"].dtype == torch.int32 and out["found"].dtype == torch.bool
    vec.core.sync()
    if name == "A":                                       # the generic one-word kernel gives the same
        gen = make_vec(name, rule_table_entries=1)
        out2 = gen.dfs(reset_roots(gen), 1 << 20)
        for k in ("status", "counts", "state"):
            assert torch.equal(out[k], out2[k]), k
        for k in ("cursor", "first"):
            assert torch.equal(out[k].records, out2[k].records), k
        gen.core.sync()


# ----------------------------------------------------------------------------- 2. budget and resume
def _moves_padded(rec, W, width):
    """[N, width] uint8 on the GPU: the moves of records [N, rb] (255 at and above the top)."""
    n = rec[:, 2].to(torch.int64)
    b = rec[:, 16 + 8 * W:16 + 24 * W].to(torch.int64).reshape(len(rec), 2 * W, 8)
    words = sum(b[:, :, i] << (8 * i) for i in range(8))                      # little-endian u64 as int64
    k = torch.arange(width, device=rec.device)
    f = ((words[:, k // 32] >> (2 * (k % 32))) & 3).to(torch.uint8)
    return torch.where(k[None, :] < (n - 1)[:, None], f, torch.full_like(f, 255))


@pytest.mark.parametrize("budget", [1, 7, 1000])
@pytest.mark.parametrize("name", ["A", "B"])
def test_budget_and_resume(on_gpu, walks, name, budget):
    """The library's own entry point with the cursor written over the records, call after call; every
    call's counters, state, status and cursor are kept on the GPU and compared at the end."""
    ws = walks[name]
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
                            counts.data_ptr(), cur.data_ptr(), first.data_ptr())
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
        ref = np.full((len(w.trace), width), 255, np.uint8)
        for i, t in enumerate(w.trace):
            ref[i, :len(t[1])] = np.frombuffer(t[1], np.uint8)
        got = _moves_padded(h_cur[:, j], W, width).cpu().numpy()
        assert np.array_equal(got[open_], ref[n[open_]]), j                   # the walker's current path
        assert torch.equal(h_cur[~torch.from_numpy(open_).to(dev), j],
                           roots.records[j].expand(int((~open_).sum()), rb)), j
        # FOUND goes up in the call that meets the first satisfying leaf
        sat_at = next((i for i, t in enumerate(w.trace) if t[0][2] > 0), None)
        assert np.array_equal((sw & FOUND) != 0, n >= sat_at if sat_at is not None else np.zeros(K, bool)), j
    assert (totals <= (calls - 1) * budget).sum() < M and (totals <= calls * budget).all()   # calls = ceil(max / B)
    assert torch.equal(h_counts[-1], h_counts[-2])                            # the extra call added nothing
    from sparc_gym_amd.snapshot import Snapshot
    fm = Snapshot(first, roots.info).moves()
    for j, w in enumerate(ws):
        assert fm[j] == (w.first or []) and (w.first is not None or not first[j].any())


def test_continuation_through_the_python_api(on_gpu, walks):
    ws = walks["A"]
    vec = make_vec("A")
    roots = reset_roots(vec)
    out = vec.dfs(roots, 1000)
    calls = 1
    while not bool(out["done"].all()):
        out = vec.dfs(out["cursor"], 1000, state=out["state"], counts=out["counts"], first=out["first"])
        calls += 1
    assert calls == -(-max(w.counts["nodes"] for w in ws) // 1000)
    check_complete(out, roots, ws)
    again = vec.dfs(out["cursor"], 1000, state=out["state"], counts=out["counts"].clone(), first=out["first"])
    assert torch.equal(again["counts"], out["counts"]) and (again["status"] == COMPLETE).all()
    with pytest.raises(ValueError, match="counts"):
        vec.dfs(roots, 10, counts=torch.zeros((len(roots), 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="budget"):
        vec.dfs(roots, 0)
    vec.core.sync()


# ----------------------------------------------------------------------------- 3. real records
@pytest.mark.parametrize("name", ["A", "B"])
def test_written_records_are_real_records(on_gpu, walks, name):
    """first and mid-walk cursors against restore + step + snapshot, from roots with step 3."""
    vec = make_vec(name)
    R = vec.num_puzzles
    vec.reset(options={"puzzle_index": np.arange(R)})
    for _ in range(3):                                                        # no-move steps: step 3, path length 1
        vec.step(torch.full((R,), 255, dtype=torch.int64, device="cuda"))
    roots = vec.snapshot()
    f = roots.fields()
    assert (f["step"] == 3).all() and (f["path_len"] == 1).all()
    mid = vec.dfs(roots, 777)
    out = vec.dfs(mid["cursor"], 1 << 20, state=mid["state"].clone(), counts=mid["counts"].clone(),
                  first=mid["first"].records.clone())
    ws = walks[name]
    assert np.array_equal(out["counts"].cpu().numpy(), np.stack([counts_of(w) for w in ws]))
    for what, snap in (("first", out["first"]), ("cursor", mid["cursor"])):
        moves = snap.moves()
        live = [j for j in range(R) if snap.records[j].any()]
        assert len(live) >= R - 2
        vec.restore(roots)
        for t in range(max(len(m) for m in moves)):
            act = [m[t] if t < len(m) and j in live else 255 for j, m in enumerate(moves)]
            idle = torch.tensor([t >= len(m) or j not in live for j, m in enumerate(moves)], device="cuda")
            before = vec.snapshot()
            vec.step(torch.tensor(act, dtype=torch.int64, device="cuda"))
            vec.restore(before, mask=idle)                                    # finished envs stand still
        want = vec.snapshot()
        for j in live:
            assert torch.equal(snap.records[j], want.records[j]), (what, j)
            assert int(snap.fields()["step"][j]) == 3 + len(moves[j])         # the root's step plus the depth
    vec.core.sync()


# ----------------------------------------------------------------------------- 4. roots inside a tree
def test_roots_inside_a_tree(on_gpu, walks):
    from sparc_gym_amd import search
    ws = walks["A"]
    vec = make_vec("A")
    R = vec.num_puzzles
    frontier, root = reset_roots(vec), torch.arange(R, device="cuda")
    extra = np.zeros((R, 8), np.int64)
    for _ in range(3):                                                        # the depth-3 forward frontier
        out = search.expand_frontier(vec, frontier)
        ch, par = out["children"], out["parent"]
        fwd = (ch.fields()["path_len"] > frontier.fields()["path_len"][par]).nonzero().squeeze(1)
        ch, par, flags, code = ch.select(fwd), par[fwd], out["flags"][fwd], out["reward_code"][fwd]
        kids = torch.bincount(par, minlength=len(frontier))
        count = lambda r: torch.bincount(r, minlength=R).cpu().numpy()        # noqa: E731
        extra[:, 5] += count(root[kids == 0])                                 # live without a forward move
        root = root[par]
        extra[:, 0] += count(root)
        term = (flags & 1) != 0                                               # the split levels' own leaves
        if term.any():
            bits = vec.audit_records(ch.select(term))["bits"].to(torch.int64)
            sat, listed = (bits & 256) != 0, code[term] == 100
            extra[:, 1] += count(root[term])
            extra[:, 2] += count(root[term][sat])
            extra[:, 3] += count(root[term][listed])
            extra[:, 4] += count(root[term][sat & listed])
        extra[:, 6] += count(root[((flags & 2) != 0) & ~term])
        live = (flags & 3) == 0
        frontier, root = ch.select(live), root[live]
    assert len(frontier) > R
    out = vec.dfs(frontier, 1 << 20)
    assert (out["status"] == COMPLETE).all() and torch.equal(out["cursor"].records, frontier.records)
    got = torch.zeros((R, 8), dtype=torch.int64, device="cuda").index_add_(0, root, out["counts"]).cpu().numpy()
    assert np.array_equal(got + extra, np.stack([counts_of(w) for w in ws]))
    # each sub-root against the walker below its prefix
    moves = frontier.moves()
    for j in range(0, len(frontier), 5):
        w = dfs_ref.walk(vec.puzzles[int(root[j])], moves[j], max_steps=MAX_STEPS["A"], root_step=3, searches=True)
        assert np.array_equal(out["counts"][j].cpu().numpy(), counts_of(w)), j
        assert out["first"].moves()[j] == (w.first or [])
    vec.core.sync()


def test_pending_and_dead_end_roots(on_gpu, walks):
    ws = walks["A"]
    vec = make_vec("A")
    q = 3
    w = ws[q]
    target = next(iter(w.leaves))                                             # a path onto the target: pending
    dead = next(t[1] for k, t in enumerate(w.trace[1:], 1) if t[0][5] == w.trace[k - 1][0][5] + 1)
    from sparc_gym_amd.snapshot import Snapshot
    snap = Snapshot.cat([step_to(vec, q, target), step_to(vec, q, list(dead)), step_to(vec, q, [])])
    out = vec.dfs(snap, 50)
    assert out["status"].cpu().tolist() == [PENDING, COMPLETE, BUDGET]
    c = out["counts"].cpu().numpy()
    assert not c[0].any() and c[1].tolist() == [0, 0, 0, 0, 0, 1, 0, 0] and c[2, 0] == 50
    assert out["done"].cpu().tolist() == [True, True, False]
    assert torch.equal(out["cursor"].records[:2], snap.records[:2])
    vec.core.sync()


def test_undo_onto_a_start_that_is_a_gap(on_gpu):
    """A start on a gap point: from path length 2 the reference's pop is illegal (the start fails
    gaps == 0, 1024-1051), and a node there without a forward move has no legal action at all, so
    its step truncates (1195).  The walk must still come back over the start."""
    import copy
    from sparc_gym_amd import SPaRCVecEnv
    proc = copy.deepcopy(dfs_ref.pool("A")[:3])
    for p in proc:
        sx, sy = (int(v) for v in p["start_location"])
        p["obs_array"]["gaps"] = np.array(p["obs_array"]["gaps"], copy=True)
        p["obs_array"]["gaps"][sx, sy] = 1
    vec = SPaRCVecEnv(len(proc), processed=proc, traceback=True, autoreset="none", observation="compact",
                      max_steps=64)
    roots = reset_roots(vec)
    assert (roots.fields()["path_len"] == 1).all()
    ws = [dfs_ref.walk(p, max_steps=64) for p in proc]
    assert all(w.counts["nodes"] > 10 for w in ws)
    for budget in (1 << 20, 13):
        out = vec.dfs(roots, budget)
        while not bool(out["done"].all()):
            out = vec.dfs(out["cursor"], budget, state=out["state"], counts=out["counts"], first=out["first"])
        assert np.array_equal(out["counts"].cpu().numpy(), np.stack([counts_of(w) for w in ws]))
        assert torch.equal(out["cursor"].records, roots.records)
        assert out["first"].moves() == [w.first or [] for w in ws]
    vec.core.sync()


# ----------------------------------------------------------------------------- 5. undecided leaves
def _searched(leaf):
    return bool(leaf["searched"])


@pytest.fixture(scope="module")
def capped():
    """Pool A with a node cap of 1 and no region-code table: every exact-fit search is undecided."""
    vec = make_vec("A", fit_cap=1, rule_table_entries=1)
    vec._load_rules()
    vec.core.set_variant(vec.core.VARIANT_HOST_FITS, 1)
    ws = [dfs_ref.walk(p, max_steps=MAX_STEPS["A"], searches=True, undecided=_searched) for p in dfs_ref.pool("A")]
    assert [w.counts["undecided"] for w in ws] == [0, 0, 0, 0, 110, 0, 5, 34]
    return vec, reset_roots(vec), ws


def test_undecided_leaves_are_stored(on_gpu, capped, walks):
    vec, roots, ws = capped
    out = vec.dfs(roots, 1 << 20, undecided=1024)
    want = np.stack([counts_of(w) for w in ws])
    c = out["counts"].cpu().numpy()
    assert np.array_equal(c, want) and (out["status"] == COMPLETE).all()
    assert c[:, 7].tolist() == [0, 0, 0, 0, 110, 0, 5, 34] and out["undecided_total"] == 149
    full = walks["A"]
    unsat = np.array([sum(not leaf["bits"] & 256 and not leaf["searched"] for leaf in w.leaves.values()) for w in full])
    assert np.array_equal(c[:, 2] + c[:, 7] + unsat, c[:, 1])                 # every target is accounted for
    assert out["first"].moves() == [w.first or [] for w in ws]                # the least DECIDED satisfying path
    got = sorted(zip(out["undecided_root"].cpu().tolist(), map(tuple, out["undecided"].moves())))
    assert got == sorted((j, a) for j, w in enumerate(full) for a, leaf in w.leaves.items() if leaf["searched"])
    bits = vec.audit_records(out["undecided"])["bits"].cpu().numpy().astype(np.uint16)
    for j, a, b in zip(out["undecided_root"].cpu().tolist(), out["undecided"].moves(), bits):
        assert int(b) == full[j].leaves[tuple(a)]["bits"], (j, a)
    only = vec.dfs(roots, 1 << 20)                                            # no buffer: counted, nobody stops
    assert torch.equal(only["counts"], out["counts"]) and (only["status"] == COMPLETE).all()
    vec.core.sync()


def test_undecided_overflow_resumes_at_the_leaf(on_gpu, capped, walks):
    vec, roots, ws = capped
    want = np.stack([counts_of(w) for w in ws])
    full = walks["A"]
    out = vec.dfs(roots, 1 << 20, undecided=16)
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
                      undecided=16)
        calls += 1
    assert calls >= -(-149 // 16)
    assert np.array_equal(out["counts"].cpu().numpy(), want)                  # nothing lost, nothing twice
    assert sorted(seen) == sorted((j, a) for j, w in enumerate(full) for a, leaf in w.leaves.items()
                                  if leaf["searched"])
    assert torch.equal(out["cursor"].records, roots.records)
    vec.core.sync()


def test_default_cap_decides_every_leaf(on_gpu, walks):
    vec = make_vec("A", rule_table_entries=1)
    out = vec.dfs(reset_roots(vec), 1 << 20, undecided=64)
    c = out["counts"].cpu().numpy()
    assert not c[:, 7].any() and out["undecided_total"] == 0 and len(out["undecided"]) == 0
    assert np.array_equal(c, np.stack([counts_of(w) for w in walks["A"]]))
    vec.core.sync()


# ----------------------------------------------------------------------------- 6. four words
def test_four_words(on_gpu):
    """Pool C's walls were put up after its solutions were found, so a stored solution may cross a
    wall: an env cannot be stepped along it.  The roots are therefore records written by hand
    (tests/record_path.py) with the trie node of the prefix: states whose path holds gap points,
    from which the reference's pop can be illegal deep inside the walk as well."""
    from record_path import encode
    from sparc_gym_amd.puzzles import build_trie
    from sparc_gym_amd.snapshot import Snapshot
    vec = make_vec("C", n=1)
    assert vec.table.words == 4
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
    roots = Snapshot(torch.from_numpy(np.stack(rows)).cuda(), info)
    assert roots.fields()["step"].cpu().tolist() == [len(pre) for _, pre in rc]
    assert any(np.asarray(vec.puzzles[q]["obs_array"]["gaps"])[pt] for q, pre in rc
               for pt in dfs_ref.points_of(vec.puzzles[q], pre))                # some prefix does cross a wall
    walkers = [dfs_ref.Walker(vec.puzzles[q], pre, root_step=len(pre), max_steps=MAX_STEPS["C"]) for q, pre in rc]
    out = vec.dfs(roots, 3000)
    for call in range(2):
        for w in walkers:
            w.run(3000)
        assert out["status"].cpu().tolist() == [COMPLETE if w.complete else BUDGET for w in walkers]
        assert np.array_equal(out["counts"].cpu().numpy(), np.stack([counts_of(w) for w in walkers]))
        assert out["cursor"].moves() == [w.path for w in walkers]
        assert out["first"].moves() == [w.first or [] for w in walkers]
        if call == 0:
            assert sum(not w.complete for w in walkers) == 4 and max(w.counts["targets"] for w in walkers) == 198
            out = vec.dfs(out["cursor"], 3000, state=out["state"], counts=out["counts"], first=out["first"])
    assert any(w.counts["nodes"] > 3000 for w in walkers)
    done = [j for j, w in enumerate(walkers) if w.complete]
    assert torch.equal(out["cursor"].records[done], roots.records[done])
    vec.core.sync()


# ----------------------------------------------------------------------------- 7. solve_dfs
@pytest.mark.parametrize("budget", [7, 4096])
@pytest.mark.parametrize("min_roots", [1, 64])
@pytest.mark.parametrize("name", ["A", "B"])
def test_solve_dfs(on_gpu, walks, name, min_roots, budget):
    from sparc_gym_amd import search
    ws = walks[name]
    vec = make_vec(name)
    res = search.solve_dfs(vec, np.arange(vec.num_puzzles), min_roots=min_roots, budget=budget)
    vec.core.sync()
    for k in NAMES:
        assert res[k].dtype == np.int64 and np.array_equal(res[k], [w.counts[k] for w in ws]), k
    assert res["complete"].all() and res["solution"] == [w.first for w in ws]
    assert res["sub_roots"] >= min(min_roots, 2) and res["launches"] >= 1
    if name == "A" and min_roots == 1 and budget == 4096:                     # and solve_by_rules agrees
        ref = search.solve_by_rules(vec, np.arange(vec.num_puzzles))
        assert [int(s.sum()) for s in ref["satisfied"]] == res["satisfied"].tolist()
        assert [len(p) for p in ref["paths"]] == res["targets"].tolist()
        assert [min((p for p, s in zip(ps, sat) if s), default=None) for ps, sat in
                zip(ref["paths"], ref["satisfied"])] == res["solution"]


def test_solve_dfs_anytime_and_undecided(on_gpu, capped, walks):
    from sparc_gym_amd import search
    vec, _, _ = capped
    full = walks["A"]
    res = search.solve_dfs(vec, np.arange(vec.num_puzzles), min_roots=8, budget=4096, undecided=16)
    for k in NAMES:                                                           # the host finished every search
        assert np.array_equal(res[k], [w.counts[k] for w in full]), k
    assert res["solution"] == [w.first for w in full] and res["complete"].all()
    part = search.solve_dfs(vec, np.arange(vec.num_puzzles), min_roots=8, budget=16, max_nodes=200)
    assert not part["complete"].all() and 200 <= part["nodes"].sum() < sum(w.counts["nodes"] for w in full)
    assert (part["targets"] <= [w.counts["targets"] for w in full]).all()
    vec.core.sync()


# ----------------------------------------------------------------------------- 8. refused arguments
def test_arguments_are_checked_before_any_launch(on_gpu):
    from sparc_gym_amd import SPaRCVecEnv
    from sparc_gym_amd._lib import SparcError
    proc = dfs_ref.pool("A")
    kw = dict(processed=proc, autoreset="none", observation="compact", max_steps=64)
    flat = SPaRCVecEnv(8, traceback=False, **kw)
    with pytest.raises(ValueError, match="traceback"):
        flat.dfs(reset_roots(flat), 10)
    flat._load_rules()
    s = reset_roots(flat)
    z = torch.zeros(8 * 64 + 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="needs a traceback context"):       # the library's own check
        flat.core.dfs_device(s.info, s.records.data_ptr(), 8, 10, z.data_ptr(), z.data_ptr(), z.data_ptr(),
                             z.data_ptr())
    vec = SPaRCVecEnv(8, traceback=True, **kw)
    s = reset_roots(vec)
    rb = s.info.record_bytes
    state = torch.zeros(8, dtype=torch.int32, device="cuda")
    status = torch.full((8,), 99, dtype=torch.uint8, device="cuda")
    counts = torch.zeros((8, 8), dtype=torch.int64, device="cuda")
    cur = torch.zeros((8, rb), dtype=torch.uint8, device="cuda")
    args = lambda **k: {**dict(info=s.info, d_records=s.records.data_ptr(), M=8, budget=10,    # noqa: E731
                               d_state=state.data_ptr(), d_status=status.data_ptr(), d_counts=counts.data_ptr(),
                               d_cursor=cur.data_ptr()), **k}
    with pytest.raises(SparcError, match="sparc_load_rules"):
        vec.core.dfs_device(**args())
    vec._load_rules()
    for bad, match in ((dict(d_records=None), "records"), (dict(d_state=None), "state"),
                       (dict(d_status=None), "status"), (dict(d_counts=None), "counts"),
                       (dict(d_cursor=None), "cursor"), (dict(M=0), "M must"), (dict(M=2**31), "M must"),
                       (dict(d_records=s.records.data_ptr() + 8), "16-B aligned"),
                       (dict(d_cursor=cur.data_ptr() + 4), "16-B aligned"),
                       (dict(d_first=cur.data_ptr() + 8), "16-B aligned"),
                       (dict(d_counts=counts.data_ptr() + 4), "8-B aligned"),
                       (dict(d_state=state.data_ptr() + 2), "4-B aligned"),
                       (dict(d_und_rec=cur.data_ptr()), "all NULL or all set"),
                       (dict(d_und_count=counts.data_ptr(), d_und_root=state.data_ptr()), "all NULL or all set")):
        with pytest.raises(ValueError, match=match):
            vec.core.dfs_device(**args(**bad))
    with pytest.raises(ValueError, match="budget"):
        vec.core.dfs_device(**args(budget=0))
    other = SPaRCVecEnv(8, traceback=True, **{**kw, "max_steps": 77})
    with pytest.raises(ValueError, match="max_steps"):
        other.dfs(s, 10)
    vec.core.sync()
    assert (status == 99).all() and not counts.any() and not state.any()      # nothing was launched


def test_bad_records_are_refused_on_the_device(on_gpu, walks):
    from sparc_gym_amd.snapshot import Snapshot
    vec = make_vec("A")
    roots = reset_roots(vec)
    rec = roots.records.clone()
    rec[1] = 0                                                                # path length 0
    rec[4, 12:16] = torch.tensor(list((99).to_bytes(4, "little")), dtype=torch.uint8, device="cuda")
    first = torch.full_like(rec, 7)
    counts = torch.full((8, 8), 5, dtype=torch.int64, device="cuda")
    out = vec.dfs(Snapshot(rec, roots.info), 1 << 20, counts=counts, first=first)
    with pytest.raises(ValueError, match="record"):
        vec.core.sync()
    vec.core.sync()                                                           # reported once
    bad = np.array([j in (1, 4) for j in range(8)])
    assert np.array_equal(out["status"].cpu().numpy(), np.where(bad, INVALID, COMPLETE))
    assert not out["cursor"].records[bad].any() and out["done"].all()
    c = out["counts"].cpu().numpy()
    assert (c[bad] == 5).all() and (first[bad] == 7).all()                    # their other outputs are untouched
    assert np.array_equal(c[~bad] - 5, np.stack([counts_of(w) for w in walks["A"]])[~bad])
    host = vec.core.dfs_host(roots.info, roots.numpy(), 1 << 20, undecided=4)  # the host-pointer form
    assert np.array_equal(host["counts"].astype(np.int64), np.stack([counts_of(w) for w in walks["A"]]))
    assert (host["status"] == COMPLETE).all() and np.array_equal(host["cursor"], roots.numpy())
    assert host["undecided_total"] == 0 and Snapshot(host["first"], roots.info).moves() == [
        w.first or [] for w in walks["A"]]
    vec.core.sync()
