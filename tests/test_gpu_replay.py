"""Replay of given action sequences on the GPU (SPaRCVecEnv.replay / roots, search.score_paths,
sparc_replay_device / _host).

Yardsticks, all made from code that is already checked against the oracle or from the reference's
own golden vectors: the golden episodes' rewards, flags and rule_status at every step; the same
sequences chained ply by ply through ``expand`` (legal mask and children) and ``select``, with the
stop rules applied in numpy (an action above 3 takes an illegal direction's child, or restore + step
+ snapshot on a second context where all four directions are legal); the C oracle stepped with the
same actions; ``playout``'s own trace; ``reset`` + ``snapshot`` for the roots.
Standing configuration of test_gpu_snapshot.py: 300 records, one full workgroup and a ragged one
whose last wave has 44 lanes; max_steps 12.  Every comparison is exact."""
import functools

import numpy as np
import pytest

import golden_io
import geometry_pools as gp
from oracle import rules_ref
from sparc_gym_amd import _lib
from sparc_gym_amd.rules import RULE_ALL
from sparc_gym_amd.search import actions_from_points, score_paths
from test_gpu_expand import MODES, _S, _ctx
from test_gpu_parity import _code
from test_gpu_playout import _pending
from test_gpu_snapshot import MAX_STEPS, N, STANDING, _arrays, _oracle, _same, _vec, _warm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

L2 = 12
END = _lib
FLAGS = [(False, False), (True, False), (False, True), (True, True)]
PER_SEQ = ("reward_code", "flags", "steps", "end", "return", "bad")
RULE_TRACE_POOLS = ("rules_7x7_tb1", "rules_mixed_tb0", "rules_tilings2w_tb1", "rules_tilings4w_tb1")


def _host(out):
    """a replay result on the host, snapshots as their records"""
    return {k: (x.records if k in ("final", "states") else x).cpu().numpy() for k, x in out.items()}


def _possible(stop_done, stop_illegal):
    """the end reasons a flag combination can produce from valid starts"""
    want = {END.REPLAY_END_EXHAUSTED}
    if stop_done:
        want |= {END.REPLAY_END_TERMINATED, END.REPLAY_END_TRUNCATED, END.REPLAY_END_PENDING}
    if stop_illegal:
        want.add(END.REPLAY_END_ILLEGAL)
    return want


# ----------------------------------------------------------------------------- the inputs of 2.
@functools.lru_cache(maxsize=None)
def standing_actions(name, tb, M=N, L=L2):
    """Action strings [L, M] over {0, 1, 2, 3, 4, 255} and ragged lengths [M] in 0..L for the
    standing records, fixed seed.  Uniform draws are rarely legal for long, so even sequences are
    and those whose record stands at step 0 are guided: a random LEGAL action of the oracle's state
    while its episode runs (the oracle is used to draw inputs only), weighted draws after it; the
    other sequences are weighted draws throughout (4 and 255 one time in sixteen each).  Sequences
    0 and 1 have length 0; the sequences from a record at step 0 have length L, the only ones that
    can take L steps under max_steps 12 with STOP_DONE."""
    S = _S(name, tb, M)
    rng = np.random.default_rng(2024)
    draw = lambda size: rng.choice(np.array([0, 1, 2, 3, 4, 255], np.uint8), p=[7 / 32] * 4 + [1 / 16] * 2,  # noqa: E731
                                   size=size)
    acts = draw((L, M))
    o = _oracle(S, autoreset="none", n=M)
    running = np.asarray(S["state"]["pending"]) == 0
    fresh = running & (np.asarray(S["state"]["step"]) == 0)
    guided = (np.arange(M) % 2 == 0) | fresh
    for t in range(L):
        legal = np.array([o.legal(i) for i in range(M)], np.int64)
        for i in np.nonzero(guided & running & (legal != 0))[0]:
            acts[t, i] = rng.choice([d for d in range(4) if legal[i] >> d & 1])
        _, f = o.rollout(1, acts[t:t + 1])
        running = running & ((f[0] & 3) == 0)
    lens = rng.integers(0, L + 1, size=M)
    lens[fresh] = L
    lens[:2] = 0
    acts.setflags(write=False)
    lens.setflags(write=False)
    return acts, lens


def oracle_replay(S, mode, acts, lens, stop_done, stop_illegal, src=None):
    """The per-sequence and per-step outputs of a replay from the standing records, by the C oracle
    stepped with the same actions (ended sequences' envs step on unobserved)."""
    L, M = acts.shape
    o = _oracle(S, src=src, autoreset=mode, n=M)
    lens = np.minimum(np.asarray(lens, np.int64), L)
    pending = np.asarray(o.state()["pending"]) != 0
    parked = pending & stop_done
    end = np.where(parked, END.REPLAY_END_PENDING, END.REPLAY_END_EXHAUSTED)
    live = ~parked & (lens > 0)
    code, flags, steps, ret = (np.zeros(M, np.int64) for _ in range(4))
    bad = np.full(M, 0xFFFF, np.int64)
    sc, sf = np.zeros((L, M), np.int64), np.zeros((L, M), np.int64)
    for t in range(L):
        if not live.any():
            break
        legal = np.array([o.legal(i) for i in range(M)], np.int64)
        a = acts[t].astype(np.int64)
        refused = live & stop_illegal & ~((a < 4) & ((legal >> np.minimum(a, 3)) & 1 != 0))
        end[refused], bad[refused] = END.REPLAY_END_ILLEGAL, t
        live = live & ~refused
        r, f = o.rollout(1, acts[t:t + 1])
        r, f = r[0].astype(np.int64), f[0].astype(np.int64)
        code, flags = np.where(live, r, code), np.where(live, f, flags)
        sc[t], sf[t] = np.where(live, r, 0), np.where(live, f, 0)
        ret, steps = ret + np.where(live, r, 0), steps + live
        term, trunc = live & stop_done & (f & 1 != 0), live & stop_done & (f & 3 == 2)
        end[term], end[trunc] = END.REPLAY_END_TERMINATED, END.REPLAY_END_TRUNCATED
        live = live & ~(term | trunc) & (steps < lens)
    return {"reward_code": code, "flags": flags, "steps": steps, "end": end, "return": ret, "bad": bad,
            "step_code": sc, "step_flags": sf}


# ----------------------------------------------------------------------------- the chained yardstick
class _Stepper:
    """restore + one step + snapshot on a second context of M envs: the step of ANY action value."""

    def __init__(self, S, mode, M):
        self.S, self.mode, self.M, self.c = S, mode, M, None

    def __call__(self, parents, acts):
        if self.c is None:
            self.c = _vec(self.S, n=self.M, autoreset=self.mode)
        c, M = self.c, self.M
        c.restore(parents)
        rew = torch.empty(M, dtype=torch.int8, device="cuda")
        flags = torch.empty(M, dtype=torch.uint8, device="cuda")
        a = torch.from_numpy(np.array(acts, np.uint8)).cuda()
        c.core.step_device(a.data_ptr(), rew.data_ptr(), flags.data_ptr())
        return c.snapshot().records.cpu().numpy(), rew.cpu().numpy(), flags.cpu().numpy()


def _chained(v, start, acts, lens, stop_done, stop_illegal, stepper):
    """The replay of `start` (a Snapshot of M records in stored form) chained ply by ply on v.expand:
    numpy arrays under the names of SPaRCVecEnv.replay's result (final [M, rb], states [L * M, rb])."""
    from sparc_gym_amd.snapshot import Snapshot
    L, M = acts.shape
    g = np.arange(M)
    cur = start.numpy().copy()
    rb = cur.shape[1]
    lens = np.minimum(np.asarray(lens, np.int64), L)
    parked = _pending(cur) & stop_done
    end = np.where(parked, END.REPLAY_END_PENDING, END.REPLAY_END_EXHAUSTED)
    live = ~parked & (lens > 0)
    code, flags, steps, ret = (np.zeros(M, np.int64) for _ in range(4))
    bad = np.full(M, 0xFFFF, np.int64)
    sc, sf = np.zeros((L, M), np.int64), np.zeros((L, M), np.int64)
    states = np.zeros((L, M, rb), np.uint8)
    for t in range(L):
        if not live.any():
            break
        parents = Snapshot(torch.from_numpy(cur).cuda(), start.info)
        out = v.expand(parents)
        legal = out["legal_mask"].cpu().numpy().astype(np.int64)
        a = acts[t].astype(np.int64)
        refused = live & stop_illegal & ~((a < 4) & ((legal >> np.minimum(a, 3)) & 1 != 0))
        end[refused], bad[refused] = END.REPLAY_END_ILLEGAL, t
        live = live & ~refused
        # an action above 3 moves nothing: the child of the lowest illegal direction is that step
        lowest_illegal = np.argmax(((legal[:, None] >> np.arange(4)) & 1) == 0, axis=1)
        a_eff = np.where(a < 4, a, lowest_illegal)
        c = out["reward_code"].cpu().numpy()[g, a_eff].astype(np.int64)
        f = out["flags"].cpu().numpy()[g, a_eff].astype(np.int64)
        child = out["children"].records.cpu().numpy()[4 * g + a_eff]
        direct = live & (a >= 4) & (legal == 15)              # no illegal direction to borrow
        if direct.any():
            rec2, c2, f2 = stepper(parents, acts[t])
            c, f = np.where(direct, c2.astype(np.int64), c), np.where(direct, f2.astype(np.int64), f)
            child = np.where(direct[:, None], rec2, child)
        code, flags = np.where(live, c, code), np.where(live, f, flags)
        sc[t], sf[t] = np.where(live, c, 0), np.where(live, f, 0)
        states[t] = np.where(live[:, None], child, 0)
        ret, steps = ret + np.where(live, c, 0), steps + live
        cur = np.where(live[:, None], child, cur)
        term, trunc = live & stop_done & (f & 1 != 0), live & stop_done & (f & 3 == 2)
        end[term], end[trunc] = END.REPLAY_END_TERMINATED, END.REPLAY_END_TRUNCATED
        live = live & ~(term | trunc) & (steps < lens)
    return {"reward_code": code, "flags": flags, "steps": steps, "end": end, "return": ret, "bad": bad,
            "step_code": sc, "step_flags": sf, "final": cur, "states": states.reshape(L * M, rb)}


def _check_against(out, ref, M, L):
    want = set(ref) if L else set(PER_SEQ) | {"final"}
    assert set(out) == want
    for k in PER_SEQ:
        assert out[k].shape == (M,) and out[k].is_cuda, k
    assert out["reward_code"].dtype == torch.int8 and out["flags"].dtype == torch.uint8
    assert out["end"].dtype == torch.uint8 and out["return"].dtype == torch.int32
    assert len(out["final"]) == M and out["final"].records.is_cuda
    if L:
        assert out["step_code"].shape == (L, M) and out["step_code"].dtype == torch.int8
        assert out["step_flags"].shape == (L, M) and out["step_flags"].dtype == torch.uint8
        assert len(out["states"]) == L * M
    got = _host(out)
    for k in want:
        assert np.array_equal(got[k], ref[k]), k


# ----------------------------------------------------------------------------- 1. golden episodes
@pytest.mark.parametrize("pool", golden_io.POOLS)
def test_golden_episodes_every_step(on_gpu, pool):
    from sparc_gym_amd import SPaRCVecEnv
    g = golden_io.load(pool)
    eps = g["episodes"]
    M = 257                                       # two workgroups, the second a single one-lane wave
    L = max(len(e["actions"]) for e in eps)
    vec = SPaRCVecEnv(1, puzzles=g["records"], traceback=g["traceback"], max_steps=g["max_steps"],
                      autoreset="none", observation="compact")
    acts = np.zeros((L, M), np.uint8)
    lens, pids = np.zeros(M, np.int64), np.zeros(M, np.int64)
    for j in range(M):
        e = eps[j % len(eps)]
        acts[:len(e["actions"]), j] = e["actions"]
        lens[j], pids[j] = len(e["actions"]), e["puzzle_index"]
    assert {4, 5, 7, 255} <= set(np.unique(acts).tolist())
    out = vec.replay(puzzle_indices=pids, actions=acts, lengths=lens, per_step=True)
    vec.core.sync()
    got = _host(out)
    fields = {k: x.cpu().numpy() for k, x in out["final"].fields().items()}
    assert (got["end"] == END.REPLAY_END_EXHAUSTED).all() and np.array_equal(got["steps"], lens)
    past_the_end = 0
    for j in range(M):
        e = eps[j % len(eps)]
        n = len(e["steps"])
        want_code = [_code(s["reward"]["value"]) for s in e["steps"]]
        assert got["step_code"][:n, j].tolist() == want_code, (pool, j)
        assert (got["step_flags"][:n, j] & 1 != 0).tolist() == [s["terminated"] for s in e["steps"]], (pool, j)
        assert (got["step_flags"][:n, j] & 2 != 0).tolist() == [s["truncated"] for s in e["steps"]], (pool, j)
        assert not got["step_code"][n:, j].any() and not got["step_flags"][n:, j].any()
        past_the_end += e["done_at"] is not None and n > e["done_at"] + 1
        last = e["steps"][-1]
        assert [fields["x"][j], fields["y"][j]] == last["info"]["agent_location"], (pool, j)
        assert fields["step"][j] == last["info"]["current_step"] and fields["puzzle_index"][j] == e["puzzle_index"]
        assert fields["path_len"][j] == len(last["visited"]["nz"]), (pool, j)   # the path never crosses itself
        assert got["reward_code"][j] == want_code[-1] and got["return"][j] == sum(want_code)
    assert past_the_end                            # episodes that step past their end are part of the fixture


# ----------------------------------------------------------------------------- 2. chained expand
@pytest.mark.parametrize("stop_done,stop_illegal", FLAGS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,tb", STANDING)
def test_replay_equals_chained_expand(on_gpu, name, tb, mode, stop_done, stop_illegal):
    S = _S(name, tb)
    v = _ctx(S, mode)
    snap = v.snapshot()
    acts, lens = standing_actions(name, tb)
    assert set(np.unique(acts).tolist()) == {0, 1, 2, 3, 4, 255}
    assert lens.min() == 0 and lens.max() == L2
    ref = _chained(v, snap, acts, lens, stop_done, stop_illegal, _Stepper(S, mode, N))
    # on the yardstick's own results: every end reason this flag combination can produce is there
    # (without STOP_DONE: no TERMINATED, TRUNCATED or PENDING; without STOP_ILLEGAL: no ILLEGAL; INVALID
    # needs a bad start: test_bad_starts_are_refused_on_the_device), a sequence takes no step, one takes L
    assert set(np.unique(ref["end"]).tolist()) == _possible(stop_done, stop_illegal)
    assert (ref["steps"] == 0).any() and (ref["steps"] == L2).any()
    if mode == "next_step" and not stop_done:
        assert (ref["step_flags"] & 64).any()      # sequences that run on into the next puzzle
    out = v.replay(snap, acts, lengths=lens, stop_done=stop_done, stop_illegal=stop_illegal, per_step=True,
                   states=True)
    _check_against(out, ref, N, L2)
    v.core.sync()
    orc = oracle_replay(S, mode, acts, lens, stop_done, stop_illegal)
    for k in orc:                                  # and, independently of expand, the C oracle
        assert np.array_equal(ref[k], orc[k]), k


# ----------------------------------------------------------------------------- 3. playout round trip
@pytest.mark.parametrize("name,tb", STANDING)
def test_a_playout_trace_replays_to_the_same_end(on_gpu, name, tb):
    K, L = 5, 6
    S = _S(name, tb)
    v = _warm(S)
    snap = v.snapshot()
    po = v.playout(snap, K, L, seed=1, forward_only=tb, trace=True, final=True)
    g = torch.arange(N * K, device="cuda")
    steps = po["steps"].reshape(-1)
    out = v.replay(snap.select(g // K), po["trace"].reshape(L, N * K), lengths=steps, stop_done=True)
    v.core.sync()
    for k in ("reward_code", "flags", "steps", "return"):
        assert torch.equal(out[k], po[k].reshape(-1)), k
    assert torch.equal(out["final"].records, po["final"].records)
    P, R = _lib, END
    maps = {P.END_TERMINATED: R.REPLAY_END_TERMINATED, P.END_TRUNCATED: R.REPLAY_END_TRUNCATED,
            P.END_HORIZON: R.REPLAY_END_EXHAUSTED, P.END_DEAD_END: R.REPLAY_END_EXHAUSTED,
            P.END_PENDING: R.REPLAY_END_PENDING}
    pe = po["end"].reshape(-1).cpu().numpy()
    assert set(np.unique(pe).tolist()) == set(maps) - ({P.END_DEAD_END} if not tb else set())
    assert np.array_equal(out["end"].cpu().numpy(), np.vectorize(maps.get)(pe))
    assert (out["bad"] == 0xFFFF).all()


# ----------------------------------------------------------------------------- 4. roots
@pytest.mark.parametrize("tb", [True, False])
@pytest.mark.parametrize("name", sorted(gp.CLASSES))
def test_roots_equal_reset_and_snapshot(on_gpu, name, tb):
    from sparc_gym_amd import SPaRCVecEnv
    proc, table, _ = gp.step_pool(name)
    P = len(proc)
    kw = dict(processed=proc, table=table, traceback=tb, max_steps=gp.MAX_STEPS, observation="compact")
    a = SPaRCVecEnv(P, **kw)
    a.reset(options={"puzzle_index": np.arange(P)})
    want = a.snapshot()
    b = SPaRCVecEnv(1, **kw)                       # loaded, never reset
    roots = b.roots(np.arange(P))
    b.core.sync()
    assert b.core.has_state is False
    assert torch.equal(roots.records, want.records)
    assert torch.equal(a.roots(torch.arange(P, device="cuda")).records, want.records)
    order = (np.arange(3 * P + 1) * 37) % P        # any number, repeats, any order
    assert torch.equal(b.roots(order).records, want.select(order).records)


# ----------------------------------------------------------------------------- 5. rule trace
@pytest.mark.parametrize("pool", RULE_TRACE_POOLS)
def test_states_audited_equal_the_reference_rule_status(on_gpu, pool):
    from sparc_gym_amd import SPaRCVecEnv
    g = golden_io.load(pool)
    eps = g["episodes"]
    M, L = len(eps), max(len(e["actions"]) for e in eps)
    vec = SPaRCVecEnv(1, puzzles=g["records"], traceback=g["traceback"], max_steps=2000, autoreset="none",
                      observation="compact")
    acts = np.full((L, M), 255, np.uint8)
    for j, e in enumerate(eps):
        acts[:len(e["actions"]), j] = e["actions"]
    lens = np.array([len(e["actions"]) for e in eps])
    out = vec.replay(puzzle_indices=[e["puzzle_index"] for e in eps], actions=acts, lengths=lens, states=True)
    t, j = np.nonzero(np.arange(L)[:, None] < lens[None, :])
    rows = t * M + j
    assert (out["states"].fields()["path_len"].cpu().numpy() > 0).tolist() == np.isin(np.arange(L * M), rows).tolist()
    bits = vec.audit_records(out["states"].select(rows))["bits"].cpu().numpy().astype(np.uint16)
    vec.core.sync()
    want = [rules_ref.rule_bits(eps[jj]["steps"][tt]["rule_status"]) for tt, jj in zip(t, j)]
    assert bits.astype(np.int64).tolist() == want
    root_bits = vec.audit_records(vec.roots([e["puzzle_index"] for e in eps]))["bits"].cpu().numpy().astype(np.uint16)
    assert root_bits.astype(np.int64).tolist() == [rules_ref.rule_bits(e["reset"]["rule_status"]) for e in eps]


# ----------------------------------------------------------------------------- 6. score_paths
def test_score_paths_on_the_listed_solutions(on_gpu):
    from sparc_gym_amd import SPaRCVecEnv
    g = golden_io.load("rules_7x7_tb1")
    vec = SPaRCVecEnv(1, puzzles=g["records"], traceback=True, max_steps=2000, autoreset="none",
                      observation="compact")                 # one env: the batch plays no part
    sol0 = {e["puzzle_index"]: e for e in g["episodes"] if e["strategy"] == "solution0"}
    q, paths, first = [], [], []
    for pi, p in enumerate(g["processed"]):
        for k, sol in enumerate(p["solution_paths"]):
            q.append(pi)
            paths.append([{"x": x, "y": y} for x, y in sol])
            first.append(k == 0)
    q, first = np.array(q), np.array(first)
    # the fixture walks solution 0 of some of its puzzles, with both verdicts among them
    verdicts = {bool(rules_ref.rule_bits(e["steps"][-1]["rule_status"]) & RULE_ALL) for e in sol0.values()}
    assert set(sol0) <= set(q[first].tolist()) and verdicts == {False, True}
    first &= np.isin(q, list(sol0))
    res = score_paths(vec, q, paths, as_points=True)
    assert vec.core.has_state is False                        # loaded, never reset
    K = len(paths)
    moves = np.array([len(p) - 1 for p in paths])
    assert res["reached"].all() and res["listed"].all() and (res["first_bad"] == -1).all()
    assert (res["end"] == END.REPLAY_END_TERMINATED).all() and np.array_equal(res["steps"], moves)
    for k in np.nonzero(first)[0]:
        e = sol0[int(q[k])]
        acts, ok = actions_from_points(g["processed"][int(q[k])]["start"], paths[k])
        assert ok and acts.tolist() == e["actions"]           # the episode IS this solution
        want = rules_ref.rule_bits(e["steps"][-1]["rule_status"])
        assert int(res["bits"][k]) == want and bool(res["satisfied"][k]) == bool(want & RULE_ALL), k
    # one move short: not reached, nothing refused
    short = score_paths(vec, q, [p[:-1] for p in paths], as_points=True)
    assert not short["reached"].any() and (short["first_bad"] == -1).all() and np.array_equal(short["steps"], moves - 1)
    assert (short["end"] == END.REPLAY_END_EXHAUSTED).all() and not short["bits"].any() and not short["satisfied"].any()
    # one move replaced by 255: refused at that index, the state that of the prefix
    at = np.array([(7 * k + 3) % m for k, m in enumerate(moves)])
    as_acts = [actions_from_points(g["processed"][int(q[k])]["start"], paths[k])[0] for k in range(K)]
    broken = [np.concatenate([a[:i], [255], a[i + 1:]]) for a, i in zip(as_acts, at)]
    br = score_paths(vec, q, broken)
    assert np.array_equal(br["first_bad"], at) and np.array_equal(br["steps"], at)
    assert (br["end"] == END.REPLAY_END_ILLEGAL).all() and not br["reached"].any() and not br["bits"].any()
    L = int(moves.max())
    pad = lambda seqs: np.stack([np.concatenate([s, np.full(L - len(s), 255)]) for s in seqs], 1).astype(np.uint8)  # noqa: E731
    stopped = vec.replay(puzzle_indices=q, actions=pad(broken), lengths=moves, stop_done=True, stop_illegal=True)
    prefix = vec.replay(puzzle_indices=q, actions=pad(as_acts), lengths=at)
    assert torch.equal(stopped["final"].records, prefix["final"].records)
    # a wrong first point: refused at index 0, no step
    moved = [[{"x": p[0]["x"] + 1, "y": p[0]["y"]}] + p[1:] for p in paths]
    wrong = score_paths(vec, q, moved, as_points=True)
    assert (wrong["first_bad"] == 0).all() and (wrong["steps"] == 0).all() and not wrong["reached"].any()
    assert (wrong["end"] == END.REPLAY_END_ILLEGAL).all()
    vec.core.sync()


# ----------------------------------------------------------------------------- 7. small shapes
@pytest.mark.parametrize("L", [0, 1, 3])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 255, 256, 257])
def test_small_shapes(on_gpu, M, L):
    S = _S("mixed_5_11", True)
    v = _warm(S)
    snap = v.snapshot().select(np.arange(M) % N)
    if L == 0:
        out = v.replay(snap)
        ref = {k: np.zeros(M, np.int64) for k in PER_SEQ}
        ref["end"] += END.REPLAY_END_EXHAUSTED
        ref["bad"] += 0xFFFF
        ref["final"] = snap.numpy()
        _check_against(out, ref, M, 0)
    else:
        full, lens = standing_actions("mixed_5_11", True)
        acts = np.ascontiguousarray(full[:L, np.arange(M) % N])
        lens = np.minimum(lens[np.arange(M) % N], L)
        for sd, si in ((False, False), (True, True)):
            ref = _chained(v, snap, acts, lens, sd, si, _Stepper(S, "next_step", M))
            out = v.replay(snap, acts, lengths=lens, stop_done=sd, stop_illegal=si, per_step=True, states=True)
            _check_against(out, ref, M, L)
    v.core.sync()


# ----------------------------------------------------------------------------- 8. refusals
@pytest.mark.parametrize("name,tb", [("7x7_full", True), ("mixed_5_11", False)])
def test_bad_starts_are_refused_on_the_device(on_gpu, name, tb):
    from sparc_gym_amd.snapshot import Snapshot
    S = _S(name, tb)
    v = _warm(S)
    snap = v.snapshot()
    acts, lens = standing_actions(name, tb)
    kw = dict(lengths=lens, stop_done=True, per_step=True, states=True)
    good = _host(v.replay(snap, acts, **kw))
    v.core.sync()
    rec = snap.records.clone()
    rows = [12, 63, 64, 299]                       # inside a wave, on both sides of a wave boundary, the ragged wave
    rec[rows] = 0
    out = _host(v.replay(Snapshot(rec, snap.info), acts, **kw))
    with pytest.raises(ValueError, match="replay"):
        v.core.sync()
    v.core.sync()                                  # the error is reported once
    bad = np.zeros(N, bool)
    bad[rows] = True
    for k in PER_SEQ + ("final",):
        assert not out[k][bad].any(), k
        assert np.array_equal(out[k][~bad], good[k][~bad]), k
    for k in ("step_code", "step_flags"):
        assert not out[k][:, bad].any() and np.array_equal(out[k][:, ~bad], good[k][:, ~bad]), k
    st, st_good = out["states"].reshape(L2, N, -1), good["states"].reshape(L2, N, -1)
    assert not st[:, bad].any() and np.array_equal(st[:, ~bad], st_good[:, ~bad])
    # a puzzle index past the table among valid neighbours (a tensor: checked by the kernel)
    P = len(S["proc"])
    pz = torch.arange(N, device="cuda") % P
    roots = v.roots(pz)
    pz[[5, 64, 299]] = torch.tensor([P, 2**31 - 1, P + 7], device="cuda")
    r = v.replay(puzzle_indices=pz, actions=acts, per_step=True)
    with pytest.raises(ValueError, match="replay"):
        v.core.sync()
    ok = v.replay(roots, acts, per_step=True)
    v.core.sync()
    r, ok = _host(r), _host(ok)
    badp = np.zeros(N, bool)
    badp[[5, 64, 299]] = True
    for k in PER_SEQ + ("final",):
        assert not r[k][badp].any() and np.array_equal(r[k][~badp], ok[k][~badp]), k
    assert not r["step_flags"][:, badp].any() and np.array_equal(r["step_code"][:, ~badp], ok["step_code"][:, ~badp])


def test_arguments_are_refused_with_a_message(on_gpu):
    S = _S("7x7_full", True)
    v = _warm(S)
    s = v.snapshot()
    acts = torch.zeros((3, N), dtype=torch.uint8, device="cuda")
    pz = torch.zeros(N, dtype=torch.int32, device="cuda")
    end = torch.zeros(N, dtype=torch.uint8, device="cuda")
    lib, ctx = v.core.lib, v.core.ctx
    import ctypes

    def call(rec=s.records.data_ptr(), puzzle=None, M=N, L=3, a=acts.data_ptr(), flags=0, **out):
        o = _lib.SparcReplayOut(**(out or {"end": end.data_ptr()}))
        return lib.sparc_replay_device(ctx, ctypes.byref(s.info), rec, puzzle, M, L, a, None, flags, ctypes.byref(o))

    for kw, what in ((dict(flags=4), "flags"), (dict(flags=1 << 31 | 1), "flags"), (dict(puzzle=pz.data_ptr()), "exactly one"),
                     (dict(rec=None), "exactly one"), (dict(rec=s.records.data_ptr() + 8), "aligned"),
                     (dict(final_rec=end.data_ptr() + 8), "aligned"), (dict(states=end.data_ptr() + 4), "aligned"),
                     (dict(steps=end.data_ptr() + 1), "aligned"), (dict(M=0), "M must"), (dict(L=65536), "L must"),
                     (dict(L=0), "L = 0"), (dict(a=None), "actions"), (dict(code=None), "at least one")):
        assert call(**kw) == -1, kw
        assert what in lib.sparc_last_error(ctx).decode(), (kw, lib.sparc_last_error(ctx))
    assert call() == 0 and call(flags=3) == 0 and call(rec=None, puzzle=pz.data_ptr()) == 0
    v.core.sync()
    assert (end == END.REPLAY_END_EXHAUSTED).all()
    other = _vec(S, traceback=False)
    for bad_call in (lambda: other.replay(s, acts), lambda: _vec(S, max_steps=MAX_STEPS + 1).replay(s, acts)):
        with pytest.raises(ValueError, match="traceback|max_steps"):
            bad_call()
    with pytest.raises(ValueError, match="traceback"):
        other.core.replay_device(s.info, s.records.data_ptr(), None, N, 3, acts.data_ptr(), d_end=end.data_ptr())


# ----------------------------------------------------------------------------- 9. no env, caller stream
def test_no_env_is_touched_and_a_caller_stream_gives_the_same_bytes(on_gpu):
    from test_gpu_streams import _Gate
    S = _S("mixed_5_11", True)
    v = _warm(S)
    snap = v.snapshot()
    acts, lens = standing_actions("mixed_5_11", True)
    kw = dict(lengths=lens, stop_done=True, stop_illegal=True, per_step=True, states=True)
    before, state = _arrays(v), v.state()
    own = _host(v.replay(snap, acts, **kw))
    v.core.sync()
    _same(_arrays(v), before)
    after = v.state()
    for k in state:
        assert np.array_equal(state[k], after[k]), k
    assert torch.equal(v.snapshot().records, snap.records)
    host = v.core.replay_host(snap.info, acts, records=snap.numpy(), lengths=lens, flags=3, per_step=True, states=True)
    for k, h in (("reward_code", "code"), ("return", "ret"), ("flags", "flags"), ("steps", "steps"), ("end", "end"),
                 ("bad", "bad"), ("step_code", "step_code"), ("step_flags", "step_flags"), ("final", "final"),
                 ("states", "states")):
        assert np.array_equal(host[h], own[k]), k
    # on a caller's stream: the true actions and records arrive behind a gate on that stream; a
    # launch on any other stream reads the poison (action 4: no move; the reset state's records)
    St = torch.cuda.Stream()
    true_a, true_r = torch.from_numpy(acts.copy()).cuda(), snap.records.clone()
    buf_a, buf_r = torch.full_like(true_a, 4), v.roots(np.zeros(N, np.int64)).records.clone()
    ln = torch.from_numpy(lens.copy()).cuda()
    torch.cuda.synchronize()
    from sparc_gym_amd.snapshot import Snapshot
    with torch.cuda.stream(St):
        gate = _Gate(St)
        buf_a.copy_(true_a, non_blocking=True)
        buf_r.copy_(true_r, non_blocking=True)
        out = v.replay(Snapshot(buf_r, snap.info), buf_a, **{**kw, "lengths": ln})
        gate.assert_closed("replay")
        assert v._bound_stream == St.cuda_stream
        St.synchronize()
        got = _host(out)
    for k in own:
        assert np.array_equal(got[k], own[k]), k
    v.core.sync()
