"""Every entry point on a caller's stream: the stream contract of sparc_set_stream.

A training loop that overlaps simulation with learning calls the library under
``with torch.cuda.stream(S)`` with S a non-blocking stream.  A launch or a copy that the library put
on another stream cannot be seen on the null stream or behind a host sync; on S it is a silent race.
These tests make the race lose every time:

* the gate: ``torch.cuda._sleep`` for about 20 ms on S (calibrated once per module; about 1,000
  times what a C call costs on the host), then an event;
* poison: every device input of the call under test holds valid-but-wrong data (actions 4 = no move,
  indices 0, the records of the reset state), and the copy that writes the true input is enqueued on
  S behind the gate; outputs the caller owns are filled with a sentinel on S behind the gate too, so a
  launch that ran ahead of the gate is overwritten; calls are chained, so each one's state comes
  from gated work before it;
* the results are copied device-to-device on S, S is synchronised (never the device), and compared
  with the C oracle, or with the chained-``expand`` yardstick (playouts) and the CPU walker (dfs).

Work on any other stream runs while the gate is still closed, reads poison or is overwritten, and the
comparison fails.  Nothing can fault: the poison is valid input."""
import ctypes
import functools
import time

import numpy as np
import pytest

import dfs_ref
import rules_trace as rt
from oracle import COracle
from test_dfs_ref import pool_c_roots
from test_gpu_bigpool import _state_equal
from test_gpu_counters64 import _table
from test_gpu_dfs import MAX_STEPS as DFS_MAX_STEPS
from test_gpu_dfs import BUDGET, COMPLETE, counts_of, make_vec
from test_gpu_exact_fit import MAX_STEPS as FIT_MAX_STEPS
from test_gpu_exact_fit import NO_TABLE
from test_gpu_exact_fit import _pool as _fit_pool
from test_gpu_exact_fit import _trace as _fit_trace
from test_gpu_playout import _check_against as _check_playout
from test_gpu_playout import _yardstick
from test_gpu_snapshot import MAX_STEPS, _copy_envs, _save_envs, _tables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GATE_MS = 20.0
SENT = 0x55
T_A, T_B, T_C, T_D, T_E = 35, 35, 4, 5, 8      # steps of the episode's segments a (given), b (drawn), c, d, e / f
SEED_B, T0_B = 11, 7
PK, PL = 3, 6                               # playouts per record, horizon


# ----------------------------------------------------------------------------- the gate
_CAL = {}


def _spin(stream, amount):
    with torch.cuda.stream(stream):
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(int(amount))
        else:                                                  # a chain of large products
            a = _CAL.setdefault("a", torch.zeros((2048, 2048), device="cuda"))
            b = _CAL.setdefault("b", torch.empty_like(a))
            for _ in range(int(amount)):
                torch.mm(a, a, out=b)


def _gate_amount(s):
    """what _spin needs for about GATE_MS, measured once with two events on the first gate's own stream
    (which that gate's caller has idle: no further stream is made for it)"""
    if "amount" not in _CAL:
        probe = 2_000_000 if hasattr(torch.cuda, "_sleep") else 8
        _spin(s, probe)
        s.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        _spin(s, probe)
        e1.record(s)
        e1.synchronize()
        _CAL["amount"] = max(1, int(probe * GATE_MS / max(e0.elapsed_time(e1), 1e-3)))
    return _CAL["amount"]


class _Gate:
    """About GATE_MS of device time on `stream`, then an event."""

    def __init__(self, stream):
        amount = _gate_amount(stream)
        self.start = torch.cuda.Event(enable_timing=True)
        self.done = torch.cuda.Event(enable_timing=True)
        self.start.record(stream)
        _spin(stream, amount)
        self.done.record(stream)
        self.host0 = time.perf_counter()

    def assert_closed(self, what):
        """`what` returned while the gate was still running on its stream."""
        host_ms = (time.perf_counter() - self.host0) * 1e3
        if not self.done.query():
            return
        self.done.synchronize()
        ms = self.start.elapsed_time(self.done)
        why = "the gate was too short" if ms < GATE_MS / 4 else "the call blocks on the stream"
        raise AssertionError(f"{what} returned after the gate had finished: {why} (the gate ran {ms:.2f} ms on the "
                             f"device; {host_ms:.2f} ms passed on the host between enqueueing it and the return)")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, copy=True, order="C"))
    return (t if dtype is None else t.to(dtype)).cuda()


def _np(t):
    return t.cpu().numpy()


class _Fed:
    """A device input: poison now, the true data by a copy that the caller enqueues behind the gate."""

    def __init__(self, true, poison):
        self.true = _dev(true)
        self.buf = torch.full_like(self.true, poison)

    def feed(self):
        self.buf.copy_(self.true, non_blocking=True)
        return self.buf


# ----------------------------------------------------------------------------- the oracle's episode
def _legal(o):
    return np.array([o.legal(i) for i in range(o.n)], np.uint8)


def _oracle_expand(o, pool, tb):
    """(reward codes [n, 4], flags [n, 4], legal masks [n]) of one step of every action from o's state"""
    n = o.n
    o4 = COracle(pool, 4 * n, tb, MAX_STEPS, autoreset=1)
    _copy_envs(o4, _save_envs(o), np.arange(4 * n) // 4)
    r, f = o4.rollout(1, (np.arange(4 * n) % 4).astype(np.uint8)[None])
    return r.reshape(n, 4), f.reshape(n, 4), _legal(o)


@functools.lru_cache(maxsize=None)
def _episode(name, tb, n=256, shift=0):
    """One oracle episode under next-step autoreset, computed once and read only: a 35 given steps,
    b 35 drawn, c 4 single steps, d 5 steps with planes, a snapshot point, e 8 steps (twice, around a
    restore), a fork by reversal, f 8 steps, and the one-ply expansion of the state after a and at the end."""
    proc, table, pool = _tables(name)
    rng = np.random.default_rng(77 + n + 1000 * shift)
    pids = (np.arange(n) * 7 + 3 + shift) % len(proc)
    acts = {k: rng.choice(np.array([0, 1, 2, 3, 0, 1, 2, 3, 4], np.uint8), size=(T, n))
            for k, T in (("a", T_A), ("c", T_C), ("d", T_D), ("e", T_E), ("f", T_E))}
    acts["b"] = _table(SEED_B, np.arange(n), T0_B + np.arange(T_B))
    o = COracle(pool, n, tb, MAX_STEPS, autoreset=1)
    o.reset(pids)
    expand = lambda: _oracle_expand(o, pool, tb)   # noqa: E731

    E = dict(name=name, tb=tb, n=n, proc=proc, table=table, pool=pool, pids=pids, acts=acts, legal0=_legal(o))
    st = np.zeros((n, 4), np.int32)
    E["a"] = o.rollout(T_A, acts["a"], stats=st)
    E["xa"] = expand()
    E["b"] = o.rollout(T_B, None, seed=SEED_B, t0=T0_B, stats=st)
    E["stats_ab"] = st
    assert np.array_equal(_oracle_b_given(pool, n, tb, pids, acts)[0], E["b"][0])     # the drawn actions, given
    E["c"] = o.rollout(T_C, acts["c"])
    E["d"] = o.rollout_obs(T_D, table.x_max, table.y_max, acts["d"])
    E["state_d"], E["legal_d"] = o.state(), _legal(o)
    saved = _save_envs(o)
    E["e"] = o.rollout(T_E, acts["e"])
    _copy_envs(o, saved)
    again = o.rollout(T_E, acts["e"])
    assert np.array_equal(again[0], E["e"][0]) and np.array_equal(again[1], E["e"][1])
    E["src"] = n - 1 - np.arange(n)
    _copy_envs(o, _save_envs(o), E["src"])
    E["legal_fork"] = _legal(o)
    E["f"] = o.rollout(T_E, acts["f"])
    E["state_f"] = o.state()
    E["xf"] = expand()
    # a masked fork: env i with mask[i] takes the state of env (i + 65) % n, the others keep theirs
    E["mask"], E["src_m"] = (np.arange(n) % 3 == 0).astype(np.uint8), ((np.arange(n) + 65) % n).astype(np.int32)
    _copy_envs(o, _save_envs(o), np.where(E["mask"] != 0, E["src_m"], np.arange(n)))
    E["state_m"], E["legal_m"] = o.state(), np.where(E["mask"] != 0, _legal(o), 0)
    assert not np.array_equal(E["state_m"]["pid"], E["state_f"]["pid"])
    unmasked = _save_envs(o)
    _copy_envs(o, unmasked, E["src_m"])
    assert not np.array_equal(o.state()["pid"], E["state_m"]["pid"])      # all-ones poison gives another state
    for k in ("a", "b", "e", "f"):
        assert (E[k][1] & 3).any() and (E[k][1] & 64).any(), k                # episodes end and autoreset in each
    return E


def _oracle_b_given(pool, n, tb, pids, acts):
    o = COracle(pool, n, tb, MAX_STEPS, autoreset=1)
    o.reset(pids)
    o.rollout(T_A, acts["a"])
    return o.rollout(T_B, acts["b"])


def _make(E, **kw):
    from sparc_gym_amd import SPaRCVecEnv
    args = dict(processed=E["proc"], table=E["table"], traceback=E["tb"], max_steps=MAX_STEPS, autoreset="next_step",
                observation="compact")
    args.update(kw)
    return SPaRCVecEnv(E["n"], **args)


def _same_rf(got, want, what):
    r, f = (got["reward_code"], got["flags"]) if isinstance(got, dict) else got
    assert np.array_equal(_np(r), want[0]), f"{what}: reward codes"
    assert np.array_equal(_np(f), want[1]), f"{what}: flags"


def _same_step(res, want_r, want_f, what):
    _, reward, term, trunc, info = res
    assert np.array_equal(_np(info["reward_code"]), want_r), f"{what}: reward code"
    assert np.array_equal(_np(reward), want_r.astype(np.float64) / 100.0), f"{what}: reward"
    assert np.array_equal(_np(term), (want_f & 1) != 0) and np.array_equal(_np(trunc), (want_f & 2) != 0), what
    assert np.array_equal(_np(info["legal_mask"]), (want_f >> 2) & 15), f"{what}: legal mask"
    assert np.array_equal(_np(info["autoreset"]), (want_f & 64) != 0), f"{what}: autoreset"


def _same_expand(out, want, what):
    assert np.array_equal(_np(out["reward_code"]), want[0]), f"{what}: reward codes"
    assert np.array_equal(_np(out["flags"]), want[1]), f"{what}: flags"
    assert np.array_equal(_np(out["legal_mask"]), want[2]), f"{what}: legal mask"


# ----------------------------------------------------------------------------- 1. the whole API on a caller stream
@pytest.mark.parametrize("name,tb,n", [("7x7_full", True, 256), ("7x7_full", False, 256), ("mixed_5_11", True, 256),
                                       ("15x15", True, 256), ("7x7_full", True, 300), ("mixed_5_11", False, 300)])
def test_whole_api_on_a_caller_stream(on_gpu, name, tb, n):
    """256 envs, 35 steps: the split kernel for 32 steps and the per-wave kernel for the 3-step tail,
    two launches with the pointers advanced between them; 300 envs: the ragged per-wave kernels."""
    E = _episode(name, tb, n)
    acts = E["acts"]
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        v = _make(E)
        _, info = v.reset(options={"puzzle_index": E["pids"]})            # synchronous by design: results only
        assert np.array_equal(_np(info["legal_mask"]), E["legal0"])
    fa, fd, fe, ff = (_Fed(acts[k], 4) for k in ("a", "d", "e", "f"))
    fc0 = _Fed(acts["c"][0], 4)
    src, src_m, mask = _Fed(E["src"].astype(np.int32), 0), _Fed(E["src_m"], 0), _Fed(E["mask"], 1)
    X, Y = v.x_dim, v.y_dim
    planes = torch.empty((2, n, X, Y), dtype=torch.int32, device="cuda")
    pid_d = torch.empty(n, dtype=torch.int32, device="cuda")
    rew_b = torch.empty((T_B, n), dtype=torch.int8, device="cuda")
    flg_b = torch.empty((T_B, n), dtype=torch.uint8, device="cuda")
    ra_out = torch.empty((6, n), dtype=torch.uint8, device="cuda")
    stats = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                                              # the set-up; no gate is up yet

    # ---- first gated section: rollouts with given and with drawn actions, steps from a tensor and from numpy
    with torch.cuda.stream(S):
        g = _Gate(S)
        for o in (rew_b, flg_b, ra_out):
            o.fill_(SENT)
        out_a = v.rollout(T_A, fa.feed(), stats=stats)
        out_b = v.rollout(T_B, None, seed=SEED_B, t0=T0_B, out=(rew_b, flg_b), stats=stats)
        v.random_actions(6, seed=5, t0=9, out=ra_out)
        g.assert_closed("rollout + rollout + random_actions")
        steps = [v.step(fc0.feed().to(torch.int64))]
        steps += [v.step(acts["c"][k].astype(np.int64)) for k in (1, 2, 3)]    # both pinned buffers, one reused
        kept = [t.clone() for t in (rew_b, flg_b, ra_out, stats)]
    S.synchronize()
    _same_rf(out_a, E["a"], "rollout(given)")
    _same_rf(kept[:2], E["b"], "rollout(drawn)")
    assert np.array_equal(_np(kept[2]), _table(5, np.arange(n), 9 + np.arange(6))), "random_actions"
    assert np.array_equal(_np(kept[3]), E["stats_ab"]), "stats"
    for k in range(T_C):
        _same_step(steps[k], E["c"][0][k], E["c"][1][k], f"step {k}")

    # ---- second gated section: planes, snapshot / restore / fork, expand, playout
    with torch.cuda.stream(S):
        warm = v.snapshot()                                               # each kernel once before the gate; none
        v.restore(warm)                                                   # of these calls changes the state
        v.fork(torch.arange(n, dtype=torch.int32, device="cuda"), mask=torch.ones(n, dtype=torch.uint8, device="cuda"))
        v.expand(warm)
        v.playout(warm, PK, PL, seed=1, trace=True, final=True)
        v.core.obs_pack_device(planes[0].data_ptr(), planes[1].data_ptr(), X, Y)
        S.synchronize()
        g = _Gate(S)
        planes.fill_(SENT)
        pid_d.fill_(SENT)
        out_d = v.rollout(T_D, fd.feed(), obs=True)
        v.core.obs_pack_device(planes[0].data_ptr(), planes[1].data_ptr(), X, Y)
        v.core.copy_state_device(4, pid_d.data_ptr())
        packed = (planes.clone(), pid_d.clone())
        snap = v.snapshot()
        out_e = v.rollout(T_E, fe.feed())
        _, info_r = v.restore(snap)
        out_e2 = v.rollout(T_E, fe.buf)
        _, info_f = v.fork(src.feed())
        out_f = v.rollout(T_E, ff.feed())
        end = v.snapshot()
        out_x = v.expand(end)
        out_p = v.playout(end, PK, PL, seed=1, trace=True, final=True)
        _, info_m = v.fork(src_m.feed(), mask=mask.feed())
        g.assert_closed("the second section's calls")
    S.synchronize()
    _same_rf(out_d, E["d"][:2], "rollout(obs)")
    assert np.array_equal(_np(out_d["visited"]), E["d"][2]) and np.array_equal(_np(out_d["agent_location"]), E["d"][3])
    _same_rf(out_e, E["e"], "rollout after snapshot")
    assert np.array_equal(_np(info_r["legal_mask"]), E["legal_d"]), "restore"
    _same_rf(out_e2, E["e"], "rollout after restore")
    assert np.array_equal(_np(info_f["legal_mask"]), E["legal_fork"]), "fork"
    _same_rf(out_f, E["f"], "rollout after fork")
    _same_expand(out_x, E["xf"], "expand")
    assert np.array_equal(_np(packed[0][0]), E["d"][2][-1]) and np.array_equal(_np(packed[0][1]), E["d"][3][-1]), "obs_pack"
    assert np.array_equal(_np(packed[1]), E["state_d"]["pid"]), "copy_state"
    assert np.array_equal(_np(info_m["legal_mask"]), E["legal_m"]), "masked fork"
    assert np.array_equal(_np(info_m["restored"]), E["mask"] != 0)

    # ---- calls that synchronise by design: results only
    with torch.cuda.stream(S):
        _state_equal(v.state(), E["state_m"], v.table)
        assert np.array_equal(v.current_puzzle_indices(), E["state_m"]["pid"])
        assert v._bound_stream == S.cuda_stream
        _check_playout(out_p, _yardstick(v, end, PK, PL, 1, 0, False), n, PK, PL)
        v.core.sync()


RULE_CASES = [("tilings", "default", None, 1), ("tilings", "generic", None, 1), ("tilings", "search", 1, 1),
              ("C", "default", None, 2), ("D", "default", None, 4)]
T_R1 = 12                                   # steps of the rule rollout; the rest of the trace runs without rules


@functools.lru_cache(maxsize=None)
def _rule_case(pool):
    """(processed puzzles, max_steps, pids, actions [T, n], reset-state bits [n], oracle bits [T, n]), no
    autoreset: the crafted tilings of test_gpu_exact_fit.py (one word), or pool C (two words) / D (four) of
    rules_trace.py.  On the oracle alone: the bits at reset, after T_R1 steps and at the end differ in
    at least 16 envs, so an audit that read an earlier state or poisoned records gives other bits."""
    if pool == "tilings":
        pids, acts, first, want, _ = _fit_trace("rules_tilings_tb1")
        proc, ms = _fit_pool("rules_tilings_tb1")[1], FIT_MAX_STEPS
    else:
        proc, _, rules = rt.pool(pool)
        n, T, ms = 300, 24, rt.POOLS[pool][2]
        pids = rt.puzzle_indices(n, len(proc))
        acts = rt.actions(proc, pids, T, seed=5)
        want = rt.oracle_trace(pool, n, T, True, "none", acts)["bits"]
        first = np.array([rules.bits(int(q), [proc[int(q)]["start_location"]], proc[int(q)]["start_location"])
                          for q in pids], np.int16)
    for x, y in ((first, want[-1]), (want[T_R1 - 1], want[-1]), (first, want[T_R1 - 1])):
        assert (x != y).sum() >= 16
    return proc, ms, pids, acts, first, want


@pytest.mark.parametrize("pool,kernel,cap,words", RULE_CASES, ids=[f"{p}-{k}-fit_cap={c}-W{w}" for p, k, c, w in RULE_CASES])
def test_rule_audits_on_a_caller_stream(on_gpu, pool, kernel, cap, words):
    """rollout(rules=True) (k_rollout1r, the generic kernel, W = 1, 2, 4), rule_audit (k_rules<W>),
    audit_records and the host forms, each behind a gate of its own with something that differs behind
    it: the rule rollout's actions; for rule_audit a rollout without rules (asynchronous) before it, so
    a k_rules launch that ran ahead reads the state of T_R1 steps earlier; for audit_records true
    records copied over the reset state's records; for rules_host a restore of the earlier state; for
    rules_records_host two calls with different records, so a piece that ran ahead meets the previous
    call's scratch.  With fit_cap = 1 and no region-code table every exact fit is queued and
    sparc_rules_finish's queue read and host finish run on S as well."""
    from sparc_gym_amd import SPaRCVecEnv
    from sparc_gym_amd.snapshot import Snapshot
    proc, ms, pids, acts, first, want = _rule_case(pool)
    T, n = acts.shape
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        kw = dict(fit_cap=cap, **({"rule_table_entries": NO_TABLE} if kernel == "search" else {}))
        vec = SPaRCVecEnv(n, processed=proc, traceback=True, autoreset="none", observation="compact", rules=True,
                          max_steps=ms, **kw)
        assert vec.table.words == words
        if kernel == "generic":
            vec.core.set_variant(vec.core.VARIANT_RULE_ROLLOUT_GENERIC, 1)
        _, info = vec.reset(options={"puzzle_index": pids})
        queued = vec.core.rules_queue_stats()["last_searches"]
        assert np.array_equal(_np(info["rule_bits"]), first)
        reset_rec = vec.snapshot().records.clone()                         # the poison of the records audit
    f1, f2 = _Fed(acts[:T_R1], 4), _Fed(acts[T_R1:], 4)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        _Gate(S)
        out = vec.rollout(T_R1, f1.feed(), rules=True)                     # ends in sparc_rules_finish: synchronous
        queued += vec.core.rules_queue_stats()["last_searches"]
        bits = out["rule_bits"].clone()
        early = vec.snapshot()                                             # the state after T_R1 steps
        S.synchronize()
        g = _Gate(S)
        vec.rollout(T - T_R1, f2.feed(), record=False)
        g.assert_closed("rollout before rule_audit")
        audit = {k: t.clone() for k, t in vec.rule_audit(fit=True).items()}
        late = vec.snapshot()
        buf = reset_rec.clone()
        S.synchronize()
        g = _Gate(S)
        buf.copy_(late.records, non_blocking=True)
        g.assert_closed("the copy of the true records")
        rec = vec.audit_records(Snapshot(buf, late.info), fit=True)
        assert vec._bound_stream == S.cuda_stream
        early_np, late_np = early.numpy(), late.numpy()
        g = _Gate(S)
        vec.core.restore_device(early.info, early.records.data_ptr(), n)   # the core's: no audit of its own
        g.assert_closed("restore_device before rules_host")
        host = vec.core.rules_host()
        _Gate(S)
        host_rec1 = vec.core.rules_records_host(late.info, early_np)
        _Gate(S)
        host_rec2 = vec.core.rules_records_host(late.info, late_np, fit=True)
    S.synchronize()
    assert np.array_equal(_np(bits), want[:T_R1]), "rule bits of the rollout"
    assert np.array_equal(_np(audit["bits"]), want[-1]), "rule_audit"
    assert np.array_equal(_np(rec["bits"]), want[-1]), "audit_records"
    assert np.array_equal(_np(audit["fit"]), _np(rec["fit"]))
    assert np.array_equal(host["bits"].astype(np.int16), want[T_R1 - 1]), "rules_host"
    assert np.array_equal(host_rec1["bits"].astype(np.int16), want[T_R1 - 1]), "rules_records_host"
    assert np.array_equal(host_rec2["bits"].astype(np.int16), want[-1]), "rules_records_host"
    assert np.array_equal(host_rec2["fit"].astype(np.int64), _np(rec["fit"]))
    if pool == "tilings":
        assert (queued > 0) == (kernel == "search")


def _pool_c_roots(vec):
    """(records [16, record_bytes] uint8, walkers) of pool C's roots, written by hand with the trie node
    of the prefix as test_gpu_dfs.py::test_four_words does: a stored solution may cross a wall, so no
    env can be stepped along it."""
    from record_path import encode
    from sparc_gym_amd.puzzles import build_trie
    info, rows, walkers = vec.core.snapshot_info(), [], []
    for q, pre in pool_c_roots():
        p = vec.puzzles[q]
        nodes, valid = build_trie(tuple(int(v) for v in p["start_location"]), p["solution_paths"][:p["solution_count"]])
        node = 0
        for a in pre:
            node = nodes[node][a]
        assert valid and node != 0xFFFF
        rows.append(encode(info, q, dfs_ref.points_of(p, pre), step=len(pre), aux=node | (nodes[node][5] << 19)))
        walkers.append(dfs_ref.Walker(p, pre, root_step=len(pre), max_steps=DFS_MAX_STEPS["C"]))
    return np.stack(rows), walkers


def test_dfs_four_words_on_a_caller_stream(on_gpu):
    """k_dfs<4>: pool C's hand-written roots, two launches of 3000 nodes, the second resumed in place
    from the first one's cursor, state and counters, behind one gate.  The poison is the records of
    other roots (the rows rolled by one): valid input, whose walks stand on another path in every row."""
    from sparc_gym_amd.snapshot import Snapshot
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        vec = make_vec("C", n=1)
        assert vec.table.words == 4
        vec.reset(options={"puzzle_index": np.zeros(1, np.int64)})           # a public method: binds the core to S
        assert vec._bound_stream == S.cuda_stream
        vec._load_rules()
        info, rb = vec.core.snapshot_info(), vec.core.snapshot_info().record_bytes
        rows, walkers = _pool_c_roots(vec)
        M = len(rows)
        assert (rows != np.roll(rows, 1, axis=0)).any(axis=1).all()           # every row's poison is another root
        fed = _Fed(rows, 0)
        fed.buf.copy_(fed.true.roll(1, 0))
        cur = fed.buf
        state = torch.zeros(M, dtype=torch.int32, device="cuda")
        counts = torch.zeros((M, 8), dtype=torch.int64, device="cuda")
        first = torch.zeros((M, rb), dtype=torch.uint8, device="cuda")
        status = torch.empty((2, M), dtype=torch.uint8, device="cuda")
    want_status, want_counts = [], []
    for _ in range(2):
        for w in walkers:
            w.run(3000)
        want_status.append([COMPLETE if w.complete else BUDGET for w in walkers])
        want_counts.append(np.stack([counts_of(w) for w in walkers]))
    assert want_status[0].count(BUDGET) == 4 and any(w.counts["nodes"] > 3000 for w in walkers)   # work was left
    assert (want_counts[1] != np.roll(want_counts[1], 1, axis=0)).any(axis=1).sum() >= 12   # other roots count otherwise
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        g = _Gate(S)
        fed.feed()
        status.fill_(SENT)
        for k in range(2):
            vec.core.dfs_device(info, cur.data_ptr(), M, 3000, state.data_ptr(), status[k].data_ptr(),
                                counts.data_ptr(), cur.data_ptr(), first.data_ptr())
        g.assert_closed("two dfs_device launches")
        kept = [t.clone() for t in (cur, counts, first, status)]
    S.synchronize()
    cur2, counts2, first2, status2 = kept
    assert _np(status2).tolist() == want_status
    assert np.array_equal(_np(counts2), want_counts[1])
    assert Snapshot(cur2, info).moves() == [w.path for w in walkers]
    assert Snapshot(first2, info).moves() == [w.first or [] for w in walkers]
    done = [j for j, w in enumerate(walkers) if w.complete]
    assert torch.equal(cur2[done], fed.true[done])                        # the true roots again, byte for byte
    with torch.cuda.stream(S):
        vec.core.sync()


@pytest.mark.parametrize("name,words", [("A", 1), ("B", 2)])
def test_dfs_on_a_caller_stream(on_gpu, name, words):
    """Two budgeted launches, the second resumed from the first one's cursor, state and counters, all
    behind one gate.  The true roots have step 3 (three no-move steps); the poison is the reset state's
    records, whose walks count the same nodes but end on a cursor with step 0.  (The four-word pool:
    test_dfs_four_words_on_a_caller_stream.)"""
    ws = dfs_ref.complete_walks(name, max_steps=DFS_MAX_STEPS[name], **({"searches": True} if name == "A" else {}))
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        vec = make_vec(name)
        assert vec.table.words == words
        vec._load_rules()
        M = vec.num_puzzles
        vec.reset(options={"puzzle_index": np.arange(M)})
        poison = vec.snapshot().records.clone()
        for _ in range(3):
            vec.step(torch.full((M,), 255, dtype=torch.int64, device="cuda"))
        roots = vec.snapshot()
        assert (roots.fields()["step"] == 3).all() and not torch.equal(roots.records, poison)
        info, rb = roots.info, roots.info.record_bytes
        cur = poison.clone()
        state = torch.zeros(M, dtype=torch.int32, device="cuda")
        counts = torch.zeros((M, 8), dtype=torch.int64, device="cuda")
        first = torch.zeros((M, rb), dtype=torch.uint8, device="cuda")
        status = torch.empty((2, M), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        g = _Gate(S)
        cur.copy_(roots.records, non_blocking=True)
        status.fill_(SENT)
        for k, budget in enumerate((777, 1 << 20)):
            vec.core.dfs_device(info, cur.data_ptr(), M, budget, state.data_ptr(), status[k].data_ptr(),
                                counts.data_ptr(), cur.data_ptr(), first.data_ptr())
        g.assert_closed("two dfs_device launches")
        kept = [t.clone() for t in (cur, state, counts, first, status)]
    S.synchronize()
    cur2, state2, counts2, first2, status2 = kept
    totals = np.array([w.counts["nodes"] for w in ws])
    assert (totals > 777).any()                                            # the second launch had work left
    assert np.array_equal(_np(counts2), np.stack([counts_of(w) for w in ws]))
    assert np.array_equal(_np(status2[0]) == COMPLETE, totals <= 777) and (_np(status2[1]) == COMPLETE).all()
    assert torch.equal(cur2, roots.records)                                # the true roots again, step 3
    from sparc_gym_amd.snapshot import Snapshot
    fs = Snapshot(first2, info)
    for j, (w, m) in enumerate(zip(ws, fs.moves())):
        assert m == (w.first or []) and (w.first is not None or not first2[j].any())
        if w.first is not None:
            assert int(fs.fields()["step"][j]) == 3 + len(m)
    with torch.cuda.stream(S):
        _Gate(S)                                                           # the host form: results only
        host = vec.core.dfs_host(info, roots.numpy(), 1 << 20)
        vec.core.sync()
    assert np.array_equal(host["counts"].astype(np.int64), _np(counts2)) and (host["status"] == COMPLETE).all()
    assert np.array_equal(host["cursor"], roots.numpy()) and np.array_equal(host["first"], _np(first2))


def test_host_forms_on_a_caller_stream(on_gpu):
    """step_host, snapshot_host, restore_host, expand_host and playout_host stage through the
    context's scratch with copies and launches on its stream and then wait for it.  Each call is made
    behind a gate of its own, after a gated rollout, with inputs that differ from the previous
    call's, so a piece on another stream meets the previous call's scratch.  Results only."""
    from sparc_gym_amd.snapshot import Snapshot
    E = _episode("7x7_full", True, 300)
    n, acts = 300, E["acts"]
    o = COracle(E["pool"], n, True, MAX_STEPS, autoreset=1)
    o.reset(E["pids"])
    o.rollout(T_A, acts["a"])
    want = {"c0": o.rollout(1, acts["c"][:1])}
    saved, want["legal"], want["x"] = _save_envs(o), _legal(o), _oracle_expand(o, E["pool"], True)
    want["c1"] = o.rollout(1, acts["c"][1:2])
    _copy_envs(o, saved)
    want["c2"] = o.rollout(1, acts["c"][2:3])
    # one env in one round trip: env 5 steps alone after segment e, env 7 is read after segment f
    o.rollout(T_E, acts["e"])
    one = COracle(E["pool"], 1, True, MAX_STEPS, autoreset=1)
    _copy_envs(one, _save_envs(o), [5])
    want["env_step"] = one.rollout(1, acts["c"][3:4, 5:6]), one.state()
    ctypes.memmove(ctypes.byref(o.envs[5]), ctypes.byref(one.envs[0]), ctypes.sizeof(one.envs[0]))
    o.rollout(T_E, acts["f"])
    want["env_read"] = o.state()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        v = _make(E)
        v.reset(options={"puzzle_index": E["pids"]})
    fa, fe, ff = (_Fed(acts[k], 4) for k in ("a", "e", "f"))
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        core, info = v.core, v.core.snapshot_info()
        _Gate(S)
        v.rollout(T_A, fa.feed(), record=False)
        got = {"c0": core.step_host(acts["c"][0])}
        _Gate(S)
        rec = core.snapshot_host()
        _Gate(S)
        got["c1"] = core.step_host(acts["c"][1])
        _Gate(S)
        flags = core.restore_host(info, rec)
        _Gate(S)
        got["c2"] = core.step_host(acts["c"][2])
        _Gate(S)
        children, xr, xf, xp = core.expand_host(info, rec)
        _Gate(S)
        play = core.playout_host(info, rec, PK, PL, seed=1, trace=True, final=True)
        snap = Snapshot(torch.from_numpy(rec).cuda(), info)
        ref = _yardstick(v, snap, PK, PL, 1, 0, False)
        dev_children = _np(v.expand(snap)["children"].records)
        g = _Gate(S)
        v.rollout(T_E, fe.feed(), record=False)
        g.assert_closed("rollout before env_step")
        stepped = core.env_step(int(acts["c"][3, 5]), env=5)
        g = _Gate(S)
        v.rollout(T_E, ff.feed(), record=False)
        g.assert_closed("rollout before env_read")
        read = core.env_read(env=7)
        v.core.sync()
    (r1, f1), s1 = want["env_step"]
    assert (stepped.reward_code, stepped.flags & 3) == (int(r1[0, 0]), int(f1[0, 0]) & 3), "env_step"
    for rec, st, i in ((stepped, s1, 0), (read, want["env_read"], 7)):
        got1 = (rec.x, rec.y, rec.path_len, rec.step, rec.puzzle, rec.pending)
        assert got1 == tuple(int(st[k][i]) for k in ("x", "y", "path_len", "step", "pid", "pending")), (i, got1)
    for k in ("c0", "c1", "c2"):
        assert np.array_equal(got[k][0], want[k][0][0]) and np.array_equal(got[k][1], want[k][1][0]), k
    assert np.array_equal((flags >> 2) & 15, want["legal"]), "restore_host"
    assert np.array_equal(xr, want["x"][0]) and np.array_equal(xf, want["x"][1]), "expand_host"
    assert np.array_equal((xp >> 2) & 15, want["x"][2]) and np.array_equal(children, dev_children)
    for k, h in (("reward_code", "code"), ("return", "ret"), ("flags", "flags"), ("steps", "steps"), ("first", "first"),
                 ("end", "end"), ("trace", "trace"), ("final", "final"), ("stats", "stats")):
        assert np.array_equal(play[h], ref[k]), f"playout_host {k}"


# ----------------------------------------------------------------------------- 2. "asynchronous" is asynchronous
ASYNC = ["rollout", "rollout_drawn", "rollout_obs", "step_gym", "random_actions", "snapshot_device",
         "restore_device", "fork_device", "expand_device", "playout_device", "dfs_device", "copy_state_device",
         "obs_pack_device"]


def _core_calls(v):
    """One call of each entry point the header marks asynchronous, on buffers allocated here."""
    c, n, dev = v.core, v.num_envs, "cuda"
    X, Y = v.x_dim, v.y_dim
    info = c.snapshot_info()
    rb = info.record_bytes
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)   # noqa: E731
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
    acts = torch.randint(0, 4, (T_A, n), dtype=torch.uint8, device=dev)
    rew, flags, stats = torch.zeros((T_A, n), dtype=torch.int8, device=dev), u8(T_A, n), i32(n, 4)
    vis, agent = i32(T_D, n, X, Y), i32(T_D, n, X, Y)
    gym = u8(12 * n)
    rec, child, exo, cursor = u8(n, rb), u8(4 * n, rb), u8(9 * n), u8(n, rb)
    src = torch.arange(n - 1, -1, -1, dtype=torch.int32, device=dev)
    pend, pstats = u8(n * PK), i32(n, 4, 4)
    dstate, dstatus, dcounts = i32(n), u8(n), torch.zeros((n, 8), dtype=torch.int64, device=dev)
    keep = [acts, rew, flags, stats, vis, agent, gym, rec, child, exo, cursor, src, pend, pstats, dstate, dstatus, dcounts]
    p = lambda t, off=0: t.data_ptr() + off                          # noqa: E731
    calls = {
        "rollout": lambda: c.rollout_device(T_A, p(acts), p(rew), p(flags), p(stats)),
        "rollout_drawn": lambda: c.rollout_device(T_A, None, p(rew), p(flags), p(stats), seed=3, t0=4),
        "rollout_obs": lambda: c.rollout_obs_device(T_D, p(acts), p(rew), p(flags), p(stats), p(vis), p(agent), X, Y),
        "step_gym": lambda: c.step_gym_device(p(acts), 1, p(gym), p(gym, 8 * n), p(gym, 9 * n), p(gym, 10 * n),
                                              p(gym, 11 * n), p(rew), p(flags), p(vis), p(agent), X, Y, p(stats),
                                              p(stats, 4 * n)),
        "random_actions": lambda: c.random_actions_device(T_A, p(acts), seed=3, t0=4),
        "snapshot_device": lambda: c.snapshot_device(None, n, p(rec)),
        "restore_device": lambda: c.restore_device(info, p(rec), n, None, None, p(flags)),
        "fork_device": lambda: c.fork_device(p(src), None, p(flags)),
        "expand_device": lambda: c.expand_device(info, p(rec), n, p(child), p(exo), p(exo, 4 * n), p(exo, 8 * n)),
        "playout_device": lambda: c.playout_device(info, p(rec), n, PK, PL, seed=1, d_end=p(pend), d_stats=p(pstats)),
        "dfs_device": lambda: c.dfs_device(info, p(rec), n, 20, p(dstate.zero_()), p(dstatus), p(dcounts), p(cursor)),
        "copy_state_device": lambda: c.copy_state_device(4, p(stats)),
        "obs_pack_device": lambda: c.obs_pack_device(p(vis), p(agent), X, Y),
    }
    assert list(calls) == ASYNC
    return calls, keep


# dfs_device on the one-word pool only: the audits of its 7x7 target leaves are table look-ups
@pytest.mark.parametrize("name,call", [(nm, c) for nm in ("7x7_full", "mixed_5_11") for c in ASYNC
                                       if (nm, c) != ("mixed_5_11", "dfs_device")])
def test_asynchronous_entry_points_return_before_the_gate_opens(on_gpu, name, call):
    """After one warm-up call (scratch sized, kernel attributes set) the call is enqueued behind a
    running gate and must return while the gate still runs.  A failure says whether the gate was too
    short or the call blocked."""
    E = _episode(name, True, 256)
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        v = _make(E)
        v.reset(options={"puzzle_index": E["pids"]})
        if call == "dfs_device":
            v._load_rules()
        calls, keep = _core_calls(v)
        calls["snapshot_device"]()                                        # valid records for the record calls
        calls[call]()                                                     # the warm-up
        v.core.sync()
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        g = _Gate(S)
        calls[call]()
        g.assert_closed(f"sparc_{call}")
    S.synchronize()
    with torch.cuda.stream(S):
        v.core.sync()
    del keep


# ----------------------------------------------------------------------------- 3. switching streams
def test_hand_over_between_streams(on_gpu):
    """S1 (gated) -> S2 -> the default stream, each hand-over a wait_stream and nothing else: the
    context's state and scratch are ordered with the caller's streams.  One oracle episode."""
    E = _episode("7x7_full", True, 256)
    acts, n = E["acts"], 256
    S1, S2, D = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.default_stream()
    with torch.cuda.stream(S1):
        v = _make(E)
        v.reset(options={"puzzle_index": E["pids"]})
    fa, fb, fd = _Fed(acts["a"], 4), _Fed(acts["b"], 4), _Fed(acts["d"], 4)
    torch.cuda.synchronize()
    with torch.cuda.stream(S1):
        g = _Gate(S1)
        out_a = v.rollout(T_A, fa.feed())
        assert v._bound_stream == S1.cuda_stream
    S2.wait_stream(S1)
    with torch.cuda.stream(S2):
        out_b = v.rollout(T_B, fb.feed())                                 # the drawn actions of b, given
        step0 = v.step(acts["c"][0].astype(np.int64))
        assert v._bound_stream == S2.cuda_stream
    g.assert_closed("rollout on S1, wait_stream, rollout and step on S2")
    D.wait_stream(S2)
    steps = [v.step(acts["c"][k].astype(np.int64)) for k in (1, 2)] + [v.step(_dev(acts["c"][3]))]
    out_d = v.rollout(T_D, fd.feed(), obs=True)
    assert v._bound_stream == D.cuda_stream
    pid = v.current_puzzle_indices()
    st = v.state()
    torch.cuda.synchronize()                                              # the gated section ended with state()
    _same_rf(out_a, E["a"], "S1")
    _same_rf(out_b, E["b"], "S2")
    for k, res in enumerate([step0] + steps):
        _same_step(res, E["c"][0][k], E["c"][1][k], f"step {k}")
    _same_rf(out_d, E["d"][:2], "default stream")
    _state_equal(st, E["state_d"], v.table)
    assert np.array_equal(pid, E["state_d"]["pid"])


def _public_methods():
    """name -> call(v, snap): every public method of SPaRCVecEnv that touches the device"""
    n = 256
    acts = lambda T: torch.zeros((T, n), dtype=torch.uint8, device="cuda")   # noqa: E731
    return {
        "reset": lambda v, s: v.reset(options={"puzzle_index": np.zeros(n, np.int64)}),
        "step": lambda v, s: v.step(np.zeros(n, np.int64)),
        "rollout": lambda v, s: v.rollout(3, acts(3)),
        "random_actions": lambda v, s: v.random_actions(3),
        "rule_audit": lambda v, s: v.rule_audit(),
        "snapshot": lambda v, s: v.snapshot(),
        "restore": lambda v, s: v.restore(s),
        "fork": lambda v, s: v.fork(np.arange(n)),
        "expand": lambda v, s: v.expand(s),
        "playout": lambda v, s: v.playout(s, 1, 2),
        "audit_records": lambda v, s: v.audit_records(s),
        "dfs": lambda v, s: v.dfs(s, 5),
        "state": lambda v, s: v.state(),
        "current_puzzle_indices": lambda v, s: v.current_puzzle_indices(),
    }


PUBLIC = ["reset", "step", "rollout", "random_actions", "rule_audit", "snapshot", "restore", "fork", "expand",
          "playout", "audit_records", "dfs", "state", "current_puzzle_indices"]


@pytest.mark.parametrize("method", PUBLIC)
def test_every_public_method_binds_the_current_stream(on_gpu, method):
    E = _episode("7x7_full", True, 256)
    S0, X = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(S0):
        v = _make(E)
        v.reset(options={"puzzle_index": E["pids"]})
        snap = v.snapshot()
        assert v._bound_stream == S0.cuda_stream != X.cuda_stream
    X.wait_stream(S0)
    with torch.cuda.stream(X):
        _public_methods()[method](v, snap)
        assert v._bound_stream == X.cuda_stream, f"{method}() left the context on the previous stream"
        v.core.sync()


# ----------------------------------------------------------------------------- 4. two contexts, two streams
def test_two_contexts_on_two_streams_interleaved(on_gpu):
    """Context A gated on S1 and B gated on S2, on the same pool with different puzzles and actions,
    their calls interleaved from one host thread: scratch shared between contexts, or a kernel
    attribute set for one and not the other, would show in one of them."""
    EA, EB = _episode("7x7_full", True, 256), _episode("7x7_full", True, 256, 1)
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    envs = []
    for S, E in ((S1, EA), (S2, EB)):
        with torch.cuda.stream(S):
            v = _make(E)
            v.reset(options={"puzzle_index": E["pids"]})
            envs.append(v)
    A, B = envs
    fA, fB = _Fed(EA["acts"]["a"], 4), _Fed(EB["acts"]["a"], 4)
    torch.cuda.synchronize()
    with torch.cuda.stream(S1):
        gA = _Gate(S1)
    with torch.cuda.stream(S2):
        gB = _Gate(S2)
    with torch.cuda.stream(S1):
        a1 = A.rollout(T_A, fA.feed())
    with torch.cuda.stream(S2):
        b1 = B.rollout(T_A, fB.feed())
    with torch.cuda.stream(S1):
        sA = A.snapshot()
        pA = A.playout(sA, PK, PL, seed=1, trace=True, final=True)
    with torch.cuda.stream(S2):
        xB = B.expand()
    with torch.cuda.stream(S1):
        xA = A.expand(sA)
        a2 = A.rollout(T_B, None, seed=SEED_B, t0=T0_B)
    with torch.cuda.stream(S2):
        b2 = B.rollout(T_B, None, seed=SEED_B, t0=T0_B)
    gA.assert_closed("context A's calls")
    gB.assert_closed("context B's calls")
    S1.synchronize()
    S2.synchronize()
    for what, E, r1, x, r2 in (("A", EA, a1, xA, a2), ("B", EB, b1, xB, b2)):
        _same_rf(r1, E["a"], what)
        _same_expand(x, E["xa"], what)
        _same_rf(r2, E["b"], what)
    assert not np.array_equal(EA["a"][0], EB["a"][0])
    with torch.cuda.stream(S1):
        _check_playout(pA, _yardstick(A, sA, PK, PL, 1, 0, False), 256, PK, PL)
        A.core.sync()
    with torch.cuda.stream(S2):
        B.core.sync()


# ----------------------------------------------------------------------------- 5. the core
def test_core_on_a_set_stream_its_own_stream_and_the_null_stream(on_gpu):
    """A raw SparcCore: gated reset_device / rollout_device / step_device on a set stream, then its own
    stream with a host sync on both sides, then the null stream: three segments of one oracle episode."""
    from sparc_gym_amd.core import SparcCore
    E = _episode("7x7_full", True, 256)
    n, acts, dev = 256, E["acts"], "cuda"
    o = COracle(E["pool"], n, True, MAX_STEPS, autoreset=1)
    o.reset(E["pids"])
    legal0 = _legal(o)
    want = [o.rollout(T_A, acts["a"]), o.rollout(1, acts["c"][:1])]
    m_np, q_np = (np.arange(n) % 5 == 0).astype(np.uint8), ((E["pids"] + 9) % len(E["proc"])).astype(np.int32)
    for i in np.flatnonzero(m_np):                                          # a masked reset of every fifth env
        assert o.lib.oracle_reset(ctypes.byref(o.pool.c), ctypes.byref(o.envs[i]), int(q_np[i])) == 0
    legal_m = _legal(o)
    want += [o.rollout(T_B, None, seed=SEED_B, t0=T0_B), o.rollout(T_E, acts["e"])]
    core = SparcCore(E["table"], n, True, MAX_STEPS, "next_step", 0, 0)
    S = torch.cuda.Stream()
    core.set_stream(S.cuda_stream)
    pidx, fa, fc = _Fed(E["pids"].astype(np.int32), 0), _Fed(acts["a"], 4), _Fed(acts["c"][0], 4)
    fe = _dev(acts["e"])
    fq, fm = _Fed(q_np, 0), _Fed(m_np, 1)
    flags0, flags_m = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2))
    rew = [torch.empty((T, n), dtype=torch.int8, device=dev) for T in (T_A, 1, T_B, T_E)]
    flg = [torch.empty((T, n), dtype=torch.uint8, device=dev) for T in (T_A, 1, T_B, T_E)]
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        g = _Gate(S)
        for t in [flags0] + rew[:2] + flg[:2]:
            t.fill_(SENT)
        core.reset_device(pidx.feed().data_ptr(), None, flags0.data_ptr())
        core.rollout_device(T_A, fa.feed().data_ptr(), rew[0].data_ptr(), flg[0].data_ptr())
        core.step_device(fc.feed().data_ptr(), rew[1].data_ptr(), flg[1].data_ptr())
        flags_m.fill_(SENT)
        core.reset_device(fq.feed().data_ptr(), fm.feed().data_ptr(), flags_m.data_ptr())   # mask poison: all ones
        g.assert_closed("reset_device + rollout_device + step_device + masked reset_device")
        kept = [t.clone() for t in (flags0, rew[0], flg[0], rew[1], flg[1], flags_m)]
    S.synchronize()
    assert np.array_equal((_np(kept[0]) >> 2) & 15, legal0), "reset_device flags"
    _same_rf(kept[1:3], want[0], "set stream: rollout_device")
    _same_rf(kept[3:5], want[1], "set stream: step_device")
    got_m = _np(kept[5])
    assert np.array_equal((got_m[m_np != 0] >> 2) & 15, legal_m[m_np != 0]) and (got_m[m_np == 0] == SENT).all()
    core.use_own_stream()                                                  # S is idle: the host synchronised it
    core.rollout_device(T_B, None, rew[2].data_ptr(), flg[2].data_ptr(), seed=SEED_B, t0=T0_B)
    core.sync()
    _same_rf((rew[2], flg[2]), want[2], "own stream")
    core.set_stream(None)                                                  # the null stream: torch's default stream
    core.rollout_device(T_E, fe.data_ptr(), rew[3].data_ptr(), flg[3].data_ptr())
    _same_rf((rew[3], flg[3]), want[3], "null stream")
    _state_equal(core.read_state(), o.state(), E["table"])
    core.close()
