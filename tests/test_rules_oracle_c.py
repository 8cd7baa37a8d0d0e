"""The C rule-audit port (oracle/sparc_rules_oracle.c, the c3r CPU baseline's audit) against the
reference's own rule_status bits (tests/golden/rules_*.json.gz) and against oracle/rules_ref.py on
random walks over the bench's c3r pool."""
import os
import sys

import numpy as np
import pytest

from golden_io import load
from oracle import RulesCOracle, rules_ref
from rules_io import RULE_POOLS, ref_puzzle, snapshots

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("pool", RULE_POOLS)
def test_c_rules_match_reference_bits(pool):
    g = load(pool)
    puzzles = [ref_puzzle(p) for p in g["processed"]]
    co = RulesCOracle(puzzles)
    n = 0
    for e, pi, t, s in snapshots(g):
        assert co.bits(pi, s["path"], s["agent"]) == rules_ref.rule_bits(s["rule_status"]), (pool, e, t)
        n += 1
    assert n > 50


def _env_path(e):
    return [[e.path[k][0], e.path[k][1]] for k in range(e.path_len)]


@pytest.mark.parametrize("autoreset", [0, 1])
@pytest.mark.parametrize("traceback", [False, True])
def test_rollout_rules_equals_single_state_audits(traceback, autoreset):
    """COracle.rollout_rules (oracle_rollout one step at a time + oracle_rules_bits_batch) over a
    7x7 pool: the bits of every env after every step equal RulesCOracle.bits (the single-state
    call the golden vectors pin) on the oracle's own path and agent after that step; reward codes,
    flags, stats and the final state equal one plain rollout() of all T steps; and two calls that
    continue t0 equal one, with device-style drawn actions as with given ones."""
    import rules_trace as rt
    from oracle import COracle
    proc, opool, rules = rt.pool("A")
    n, T = 96, 40
    pids = rt.puzzle_indices(n, len(proc))
    acts = rt.actions(proc, pids, T, seed=11)
    a = COracle(opool, n, traceback, 24, autoreset=autoreset)
    a.reset(pids)
    sa = np.zeros((n, 4), np.int32)
    rew, flags, bits = a.rollout_rules(T, rules, acts, stats=sa)
    assert bits.dtype == np.int16 and bits.shape == (T, n)
    b = COracle(opool, n, traceback, 24, autoreset=autoreset)
    b.reset(pids)
    sb = np.zeros((n, 4), np.int32)
    rb, fb = b.rollout(T, acts, stats=sb)
    assert np.array_equal(rew, rb) and np.array_equal(flags, fb) and np.array_equal(sa, sb)
    for k, v in a.state().items():
        assert np.array_equal(v, b.state()[k]), k
    c = COracle(opool, n, traceback, 24, autoreset=autoreset)
    c.reset(pids)
    for t in range(T):
        c.rollout(1, acts[t:t + 1])
        want = [rules.bits(c.envs[i].pid, _env_path(c.envs[i]), (c.envs[i].x, c.envs[i].y)) for i in range(n)]
        assert bits[t].tolist() == want, t
    assert ((bits >> 8) & 1).sum() > 0 and len(np.unique(bits)) > 20
    # drawn actions: two calls continuing t0 == one call == plain rollout
    d = COracle(opool, n, traceback, 24, autoreset=autoreset)
    d.reset(pids)
    r1 = d.rollout_rules(17, rules, None, seed=7, env_offset=12345)
    r2 = d.rollout_rules(T - 17, rules, None, seed=7, env_offset=12345, t0=17)
    e = COracle(opool, n, traceback, 24, autoreset=autoreset)
    e.reset(pids)
    r = e.rollout_rules(T, rules, None, seed=7, env_offset=12345)
    for x, y, z in zip(r1, r2, r):
        assert np.array_equal(np.concatenate([x, y]), z)
    b.reset(pids)
    rb, fb = b.rollout(T, None, seed=7, env_offset=12345)
    assert np.array_equal(r[0], rb) and np.array_equal(r[1], fb)


@pytest.mark.parametrize("name", ["A", "C"])
def test_rollout_rules_sample_equals_python_port(name):
    """A sample of (env, step) pairs of COracle.rollout_rules equals oracle/rules_ref.py's audit of
    the oracle state after that step (next-step autoreset: reset steps are in the sample)."""
    import rules_trace as rt
    from oracle import COracle
    proc, opool, rules = rt.pool(name)
    n, T = 64, 48
    pids = rt.puzzle_indices(n, len(proc))
    acts = rt.actions(proc, pids, T, seed=12)
    o = COracle(opool, n, True, rt.POOLS[name][2], autoreset=1)
    o.reset(pids)
    rng = np.random.default_rng(13)
    checked, resets = 0, 0
    for t in range(T):
        _, flags, bits = o.rollout_rules(1, rules, acts[t:t + 1], t0=t)
        for i in rng.choice(n, size=8, replace=False):
            e = o.envs[i]
            want = rules_ref.rule_bits(rules_ref.audit(proc[e.pid], _env_path(e), (e.x, e.y)))
            assert int(bits[0, i]) == want, (t, i)
            checked += 1
            resets += int(flags[0, i] >> 6) & 1
    assert checked == 384 and resets > 0


@pytest.mark.parametrize("pool", RULE_POOLS)
def test_rollout_rules_replays_golden_episodes(pool):
    """Every golden episode's actions through COracle + rollout_rules: after every step the bits
    equal the reference's own rule_status bits, which pins step and audit together."""
    from golden_io import oracle_puzzles
    from oracle import COracle
    g = load(pool)
    eps = g["episodes"]
    rules = RulesCOracle([ref_puzzle(p) for p in g["processed"]])
    n, T = len(eps), max(len(e["actions"]) for e in eps)
    o = COracle(oracle_puzzles(g), n, g["traceback"], 2000, autoreset=0)
    o.reset([e["puzzle_index"] for e in eps])
    acts = np.zeros((T, n), np.uint8)
    for i, e in enumerate(eps):
        acts[:len(e["actions"]), i] = e["actions"]
    _, _, bits = o.rollout_rules(T, rules, acts)
    checked = 0
    for i, e in enumerate(eps):
        for t, s in enumerate(e["steps"]):
            assert int(bits[t, i]) == rules_ref.rule_bits(s["rule_status"]), (pool, i, t)
            checked += 1
    assert checked > 50


def test_c_rules_match_python_port_on_bench_pool():
    sys.path[:0] = [REPO, os.path.join(REPO, "sparc-gym_amd")]
    import bench
    from oracle.cpu_ref import CpuRefEnv
    proc = bench.make_pool(1024, *bench.CONFIGS["c3r"][:2], workers=1)[:64]
    co = RulesCOracle(proc)
    pool = [{"x_size": p["x_size"], "y_size": p["y_size"], "start": list(p["start_location"]),
             "target": list(p["target_location"]), "solution_count": p["solution_count"],
             "solution_paths": p["solution_paths"], "gaps": p["obs_array"]["gaps"]} for p in proc]
    rng = np.random.default_rng(7)
    seen = set()
    for q in range(len(proc)):
        env = CpuRefEnv(pool[q], True, 2000)
        for _ in range(40):
            _, term, trunc = env.step(int(rng.integers(4)))
            want = rules_ref.rule_bits(rules_ref.audit(proc[q], env.path, env.loc))
            assert co.bits(q, env.path, env.loc) == want, (q, env.path)
            seen.add(want)
            if term or trunc:
                break
    assert len(seen) > 8   # many different rule outcomes
