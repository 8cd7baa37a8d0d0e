"""Snapshot, restore and fork of the batched env state on the GPU, against the C oracle.

The oracle is forked on the CPU by copying its self-contained _Env structs.  Standing
configuration: 300 envs (one full workgroup and a ragged 44-lane wave), 64 synthetic puzzles,
max_steps 12, next-step autoreset, 48 random warm-up steps (rollout(48, None, seed=11)), so that
at the snapshot point some envs are pending, every env is past an autoreset and most have a path
longer than one point; each test asserts the first two on the oracle's state."""
import ctypes
import functools

import numpy as np
import pytest

import golden_io
from oracle import COracle, OraclePool, _Env
from sparc_gym_amd import synthetic
from sparc_gym_amd.puzzles import pack_table, process_puzzles
from test_gpu_parity import POOLS, oracle_pool_from_processed
from test_gpu_splitw_edges import _gap_free_pool, _snake

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, WARM, CONT, MAX_STEPS = 300, 48, 32, 12
STANDING = [(name, tb) for name in ("7x7_full", "mixed_5_11", "15x15") for tb in (True, False)]
WORDS = {"7x7_full": 1, "mixed_5_11": 2, "15x15": 4}


# ----------------------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def _tables(name):
    proc = process_puzzles(synthetic.make_puzzles(64, seed=0, **POOLS[name]))
    table = pack_table(proc)
    assert table.words == WORDS[name]
    return proc, table, OraclePool(oracle_pool_from_processed(proc))


def _copy_envs(o, saved, src=None):
    """o.envs[i] <- saved[src[i]] (the oracle's _Env structs are self-contained)."""
    for i in range(o.n):
        ctypes.memmove(ctypes.byref(o.envs[i]), ctypes.byref(saved[i if src is None else int(src[i])]),
                       ctypes.sizeof(_Env))


def _save_envs(o):
    saved = (_Env * o.n)()
    ctypes.memmove(saved, o.envs, ctypes.sizeof(saved))
    return saved


@functools.lru_cache(maxsize=None)
def _standing(name, tb, n=N, autoreset="next_step", warm=WARM):
    """The oracle's side of the standing configuration, computed once: the warmed-up structs, the
    legal masks at the snapshot point, and the continuation under explicit actions."""
    proc, table, pool = _tables(name)
    rng = np.random.default_rng(1000 + n)
    pids = (np.arange(n) * 7 + 3) % len(proc)
    acts = rng.choice(np.array([0, 1, 2, 3, 0, 1, 2, 3, 4], np.uint8), size=(CONT, n))
    o = COracle(pool, n, tb, MAX_STEPS, autoreset=int(autoreset == "next_step"))
    o.reset(pids)
    rw, fw = o.rollout(warm, None, seed=11)
    saved = _save_envs(o)
    st = o.state()
    legal = np.array([o.legal(i) for i in range(n)], np.uint8)
    ro, fo = o.rollout(CONT, acts)
    return dict(name=name, tb=tb, n=n, proc=proc, table=table, pool=pool, pids=pids, acts=acts, saved=saved,
                state=st, legal=legal, warm=(rw, fw), cont=(ro, fo), autoreset=autoreset, warm_steps=warm)


def _assert_interesting(S):
    """pending envs and envs past an autoreset are present by construction, not by luck"""
    st = S["state"]
    assert (st["pending"] != 0).any()
    if S["autoreset"] == "next_step":
        assert (st["pid"] != S["pids"]).any()


def _vec(S, n=None, **kw):
    from sparc_gym_amd import SPaRCVecEnv
    args = dict(processed=S["proc"], table=S["table"], traceback=S["tb"], max_steps=MAX_STEPS,
                autoreset=S["autoreset"], observation="compact")
    args.update(kw)
    return SPaRCVecEnv(S["n"] if n is None else n, **args)


def _warm(S, **kw):
    """A context brought to the snapshot point; its warm-up equals the oracle's."""
    v = _vec(S, **kw)
    v.reset(options={"puzzle_index": S["pids"]})
    out = v.rollout(S["warm_steps"], None, seed=11)
    assert np.array_equal(out["reward_code"].cpu().numpy(), S["warm"][0])
    assert np.array_equal(out["flags"].cpu().numpy(), S["warm"][1])
    return v


def _arrays(v):
    """The state arrays of sparc_copy_state_device, fields 0-5 (5 with traceback), on the host."""
    n, W = v.num_envs, v.table.words
    shapes = [(0, (W, n), torch.int64), (1, (n,), torch.int32), (2, (n,), torch.int32), (3, (n,), torch.int32),
              (4, (n,), torch.int32)]
    if v.traceback:
        shapes.append((5, (2 * W, n), torch.int64))
    out = {}
    for which, shape, dt in shapes:
        t = torch.empty(shape, dtype=dt, device="cuda")
        v.core.copy_state_device(which, t.data_ptr())
        out[which] = t.cpu().numpy()
    return out


def _same(a, b, cols=None):
    assert a.keys() == b.keys()
    for k in a:
        x, y = (a[k], b[k]) if cols is None else (a[k][..., cols], b[k][..., cols])
        assert np.array_equal(x, y), f"state field {k}"


def _run(v, acts):
    out = v.rollout(len(acts), torch.from_numpy(np.ascontiguousarray(acts)).cuda())
    return out["reward_code"].cpu().numpy(), out["flags"].cpu().numpy()


def _oracle(S, src=None, autoreset=None, n=None):
    n = S["n"] if n is None else n
    ar = S["autoreset"] if autoreset is None else autoreset
    o = COracle(S["pool"], n, S["tb"], MAX_STEPS, autoreset=int(ar == "next_step"))
    _copy_envs(o, S["saved"], src)
    return o


# ----------------------------------------------------------------------------- 1. round trip
@pytest.mark.parametrize("name,tb", STANDING)
def test_round_trip(on_gpu, name, tb):
    S = _standing(name, tb)
    _assert_interesting(S)
    v = _warm(S)
    s = v.snapshot()
    assert len(s) == N and s.records.shape == (N, s.info.record_bytes) and s.records.is_cuda
    before = _arrays(v)
    first = _run(v, S["acts"])
    _, info = v.restore(s)
    _same(_arrays(v), before)
    assert np.array_equal(info["legal_mask"].cpu().numpy(), S["legal"])
    assert info["restored"].all()
    second = _run(v, S["acts"])
    for a, b, c in zip(first, second, S["cont"]):
        assert np.array_equal(a, b) and np.array_equal(a, c)


# ----------------------------------------------------------------------------- 2. fork
def _fork_srcs(n):
    i = np.arange(n)
    return {"reverse": n - 1 - i, "rotate65": (i + 65) % n, "all_from_7": np.full(n, 7)}


@pytest.mark.parametrize("name,case", [("7x7_full", "reverse"), ("7x7_full", "rotate65"), ("7x7_full", "all_from_7"),
                                       ("mixed_5_11", "rotate65")])
def test_fork_is_a_simultaneous_assignment(on_gpu, name, case):
    n = 600   # more than two workgroups: the cycles cross them
    S = _standing(name, True, n)
    _assert_interesting(S)
    src = _fork_srcs(n)[case]
    v = _warm(S)
    before = _arrays(v)
    _, info = v.fork(src)
    after = _arrays(v)
    for k in before:
        assert np.array_equal(after[k], before[k][..., src]), f"state field {k}"
    assert np.array_equal(info["legal_mask"].cpu().numpy(), S["legal"][src])
    o = _oracle(S, src)
    ro, fo = o.rollout(CONT, S["acts"])
    r, f = _run(v, S["acts"])
    assert np.array_equal(r, ro) and np.array_equal(f, fo)


# ----------------------------------------------------------------------------- 3. fan-out, M != N
def test_fan_out_of_one_record(on_gpu):
    S = _standing("7x7_full", True)
    _assert_interesting(S)
    a = _warm(S)
    s = a.snapshot(envs=[5])
    assert len(s) == 1
    b = _vec(S)                        # a second context, never reset: the restore covers every env
    src = np.zeros(N, np.int64)
    _, info = b.restore(s, src=src)
    assert (info["legal_mask"].cpu().numpy() == S["legal"][5]).all()
    o = _oracle(S, np.full(N, 5))
    ro, fo = o.rollout(CONT, S["acts"])
    r, f = _run(b, S["acts"])
    assert np.array_equal(r, ro) and np.array_equal(f, fo)


@pytest.mark.parametrize("name,tb", [("7x7_full", True), ("mixed_5_11", False)])
def test_restore_520_records_into_300_envs(on_gpu, name, tb):
    big = _standing(name, tb, 520)
    S = _standing(name, tb)
    _assert_interesting(big)
    a = _warm(big)
    s = a.snapshot()
    src = np.random.default_rng(3).integers(520, size=N)
    b = _vec(S)
    b.restore(s, src=torch.from_numpy(src).cuda())        # a tensor: checked on the device
    b.core.sync()
    o = COracle(S["pool"], N, tb, MAX_STEPS, autoreset=1)
    _copy_envs(o, big["saved"], src)
    ro, fo = o.rollout(CONT, S["acts"])
    r, f = _run(b, S["acts"])
    assert np.array_equal(r, ro) and np.array_equal(f, fo)


def test_one_env(on_gpu):
    S = _standing("7x7_full", True, 1)
    v = _warm(S)
    s = v.snapshot()
    before = _arrays(v)
    first = _run(v, S["acts"])
    v.restore(s)
    _same(_arrays(v), before)
    second = _run(v, S["acts"])
    v.fork([0])
    for a, b, c in zip(first, second, S["cont"]):
        assert np.array_equal(a, b) and np.array_equal(a, c)


# ----------------------------------------------------------------------------- 4. masked restore
@pytest.mark.parametrize("name,tb", [("7x7_full", True), ("15x15", True)])
def test_masked_restore(on_gpu, name, tb):
    S = _standing(name, tb)
    _assert_interesting(S)
    v = _warm(S)
    s = v.snapshot()
    at_snapshot = _arrays(v)
    _run(v, S["acts"])
    before = _arrays(v)
    mask = np.arange(N) % 3 == 0
    _, info = v.restore(s, mask=mask)
    after = _arrays(v)
    _same(after, before, ~mask)
    _same(after, at_snapshot, mask)
    legal = info["legal_mask"].cpu().numpy()
    assert (legal[~mask] == 0).all()
    assert np.array_equal(legal[mask], S["legal"][mask])
    assert np.array_equal(info["restored"].cpu().numpy(), mask)


# ----------------------------------------------------------------------------- 5. long paths
@pytest.mark.parametrize("cells,moves", [(3, 40), (4, 70)])   # 7x7 (1 word), 9x9 (2 words)
def test_fork_of_long_paths(on_gpu, cells, moves):
    """Paths past 33 points (7x7) / 65 points (9x9): the later words of the direction stack must
    travel with the fork, or the pops after it go wrong."""
    from sparc_gym_amd import SPaRCVecEnv
    proc = _gap_free_pool(cells)
    table = pack_table(proc)
    assert table.words == (1 if cells == 3 else 2)
    X = proc[0]["x_size"]
    n, pops, tail = 300, 20, 16
    snake = _snake(X, X)[:moves]
    rng = np.random.default_rng(cells)
    walk = rng.integers(0, 4, (moves, n)).astype(np.uint8)
    walk[:, 0::2] = np.asarray(snake, np.uint8)[:, None]
    src = n - 1 - np.arange(n)
    # after the fork every env undoes the last `pops` actions of its source, then steps randomly
    back = (walk[::-1][:pops] ^ 2)[:, src]
    rest = np.concatenate([back, rng.integers(0, 4, (tail, n)).astype(np.uint8)])
    pids = np.arange(n) % len(proc)
    v = SPaRCVecEnv(n, processed=proc, table=table, traceback=True, max_steps=100000, autoreset="none",
                    observation="compact")
    v.reset(options={"puzzle_index": pids})
    _run(v, walk)
    o = COracle(oracle_pool_from_processed(proc), n, True, 100000, autoreset=0)
    o.reset(pids)
    o.rollout(moves, walk)
    assert (o.state()["path_len"][0::2] == moves + 1).all()
    saved = _save_envs(o)
    v.fork(src)
    _copy_envs(o, saved, src)
    ro, fo = o.rollout(len(rest), rest)
    r, f = _run(v, rest)
    assert np.array_equal(r, ro) and np.array_equal(f, fo)
    so = o.state()
    assert (so["path_len"][1::2] <= moves + 1 - pops + tail).all()   # the snake's copies did pop
    assert np.array_equal(v.state()["path_len"].astype(np.int64), so["path_len"])


# ----------------------------------------------------------------------------- 6. every consumer
def _twin_pair(proc, table, rules, observation):
    """A context that forks after its warm-up, and a twin that never forks: reset onto the source
    envs' puzzles and driven by the source envs' actions."""
    from sparc_gym_amd import SPaRCVecEnv
    kw = dict(processed=proc, table=table, traceback=True, max_steps=MAX_STEPS, autoreset="next_step",
              observation=observation, rules=rules)
    rng = np.random.default_rng(6)
    src = rng.integers(N, size=N)
    pids = (np.arange(N) * 7 + 3) % len(proc)
    a = SPaRCVecEnv(N, **kw)
    a.reset(options={"puzzle_index": pids})
    warm = a.random_actions(WARM, seed=11)
    a.rollout(WARM, warm)
    bits = a.rule_audit()["bits"].cpu().numpy() if rules else None
    _, info = a.fork(src)
    t = SPaRCVecEnv(N, **kw)
    t.reset(options={"puzzle_index": pids[src]})
    t.rollout(WARM, warm[:, torch.from_numpy(src).cuda()].contiguous())
    if rules:
        assert np.array_equal(info["rule_bits"].cpu().numpy(), bits[src])
        assert np.array_equal(t.rule_audit()["bits"].cpu().numpy(), bits[src])
    return a, t


@pytest.mark.parametrize("consumer", ["step", "rollout", "rollout_obs", "rollout_rules"])
def test_every_consumer_of_the_state_after_a_fork(on_gpu, consumer):
    if consumer == "rollout_rules":
        proc = process_puzzles(synthetic.make_rule_puzzles(64, seed=3, sizes=((3, 3),), break_prob=0.3))
        table = pack_table(proc)
    else:
        proc, table, _ = _tables("7x7_full")
    a, t = _twin_pair(proc, table, consumer == "rollout_rules",
                      "new" if consumer in ("step", "rollout_obs") else "compact")
    _same(_arrays(a), _arrays(t))
    T = 30 if consumer == "rollout_rules" else CONT
    acts = torch.from_numpy(np.random.default_rng(7).integers(0, 5, (T, N)).astype(np.uint8)).cuda()
    if consumer == "step":
        for k in range(4):
            ra, rt = a.step(acts[k]), t.step(acts[k])
            for x, y in zip(ra[1:4], rt[1:4]):
                assert torch.equal(x, y)
            for key in ra[0]:
                assert torch.equal(ra[0][key], rt[0][key]), key
            for key in ("legal_mask", "autoreset", "reward_code"):
                assert torch.equal(ra[4][key], rt[4][key]), key
    else:
        kw = {"rollout": {}, "rollout_obs": {"obs": True}, "rollout_rules": {"rules": True}}[consumer]
        ra, rt = a.rollout(T, acts, **kw), t.rollout(T, acts, **kw)
        assert ra.keys() == rt.keys()
        for key in ra:
            assert torch.equal(ra[key], rt[key]), key
    _same(_arrays(a), _arrays(t))


# ----------------------------------------------------------------------------- 7. files, mismatches
def test_file_round_trip_into_a_new_context(on_gpu, tmp_path):
    from sparc_gym_amd.snapshot import Snapshot
    S = _standing("mixed_5_11", True)
    _assert_interesting(S)
    a = _warm(S)
    path = tmp_path / "state.snap"
    a.snapshot().cpu().save(path)
    loaded = Snapshot.load(path)
    assert loaded.is_host and len(loaded) == N
    b = _vec(S)
    b.restore(loaded)
    _same(_arrays(b), _arrays(a))
    r, f = _run(b, S["acts"])
    assert np.array_equal(r, S["cont"][0]) and np.array_equal(f, S["cont"][1])


@pytest.mark.parametrize("what", ["table_hash", "traceback", "max_steps"])
def test_header_mismatch_is_rejected(on_gpu, what):
    S = _standing("7x7_full", True)
    s = _warm(S).snapshot()
    if what == "table_hash":       # the same pool with one puzzle exchanged
        proc = list(S["proc"])
        proc[17] = process_puzzles(synthetic.make_puzzles(1, seed=99, **POOLS["7x7_full"]))[0]
        table = pack_table(proc)
        assert (table.pitch, table.words) == (S["table"].pitch, S["table"].words)
        v = _vec(S, processed=proc, table=table)
    elif what == "traceback":
        v = _vec(S, traceback=False)
    else:
        v = _vec(S, max_steps=MAX_STEPS + 1)
    v.reset(options={"puzzle_index": S["pids"]})
    before = _arrays(v)
    with pytest.raises(ValueError, match=what):
        v.restore(s)
    with pytest.raises(ValueError, match=what):          # the library's own check
        v.core.restore_device(s.info, s.records.data_ptr(), len(s))
    v.core.sync()
    _same(_arrays(v), before)


def test_snapshot_of_a_none_context_restores_into_next_step(on_gpu):
    """autoreset belongs to the context: the pending envs of the snapshot autoreset on the next
    step (flags bit 6), as the oracle does from the copied structs with autoreset on."""
    S = _standing("7x7_full", True, N, "none", 10)
    st = S["state"]
    assert (st["pending"] != 0).any() and (st["pending"] == 0).any()
    c = _warm(S)
    d = _vec(S, autoreset="next_step")
    d.restore(c.snapshot())
    o = _oracle(S, autoreset="next_step")
    ro, fo = o.rollout(CONT, S["acts"])
    r, f = _run(d, S["acts"])
    assert np.array_equal((f[0] & 64) != 0, st["pending"] != 0)
    assert np.array_equal(r, ro) and np.array_equal(f, fo)


# ----------------------------------------------------------------------------- 8. index check
def test_bad_index_and_bad_record_are_refused_on_the_device(on_gpu):
    """The kernel compares before it dereferences: a record index equal to M and a record whose
    puzzle field holds P leave their envs unchanged and raise at the next sync; every other env
    is restored."""
    from sparc_gym_amd.snapshot import Snapshot
    S = _standing("7x7_full", True)
    v = _warm(S)
    s = v.snapshot()
    at_snapshot = _arrays(v)
    _run(v, S["acts"])
    before = _arrays(v)
    rec = s.records.clone()
    k_idx, k_rec = 77, 201
    P = len(S["proc"])
    rec[k_rec, 12:16] = torch.tensor(list(int(P).to_bytes(4, "little")), dtype=torch.uint8, device="cuda")
    src = torch.arange(N, dtype=torch.int32, device="cuda")
    src[k_idx] = N
    v.restore(Snapshot(rec, s.info), src=src)      # completes
    with pytest.raises(ValueError, match="restore"):
        v.core.sync()
    v.core.sync()                                  # the error is reported once
    after = _arrays(v)
    bad = np.zeros(N, bool)
    bad[[k_idx, k_rec]] = True
    _same(after, before, bad)
    _same(after, at_snapshot, ~bad)
    # a host-side index list is refused in Python
    with pytest.raises(ValueError):
        v.restore(s, src=np.full(N, N))
    with pytest.raises(ValueError):
        v.fork(np.arange(N - 1))
    with pytest.raises(ValueError):
        v.snapshot(envs=[N])


# ----------------------------------------------------------------------------- 9. SPaRC_Gym.snapshot
def test_drop_in_env_snapshot_fans_out(on_gpu):
    from sparc_gym_amd import SPaRC_Gym, SPaRCVecEnv
    g = golden_io.load("poolA_tb1")
    assert g["traceback"]
    ep = next(e for e in g["episodes"] if len(e["actions"]) >= 10)
    env = SPaRC_Gym(puzzles=g["records"], traceback=g["traceback"], max_steps=g["max_steps"])
    env.reset(options={"puzzle_id": ep["puzzle_id"]})
    for a in ep["actions"][:6]:
        env.step(a)
    s = env.snapshot()
    assert len(s) == 1 and s.is_host
    n = 128
    vec = SPaRCVecEnv(n, puzzles=g["records"], traceback=g["traceback"], max_steps=g["max_steps"], autoreset="none")
    _, info = vec.restore(s, src=np.zeros(n, np.int64))
    want = ep["steps"][5]["info"]["legal_actions"]
    assert all([a for a in range(4) if m >> a & 1] == want for m in info["legal_mask"].cpu().numpy())
    for a, st in zip(ep["actions"][6:], ep["steps"][6:]):
        _, rew, term, trunc, _ = vec.step(torch.full((n,), a, dtype=torch.int64, device="cuda"))
        assert (rew.cpu().numpy() == st["reward"]["value"]).all()
        assert (term.cpu().numpy() == st["terminated"]).all() and (trunc.cpu().numpy() == st["truncated"]).all()
