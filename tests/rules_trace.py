"""Pools, action streams and oracle traces for the every-env, every-step checks of the rule audit
(tests/test_gpu_rules_trace.py on the GPU, tests/test_rules_oracle_c.py for the helper itself).

The oracle side is COracle.rollout_rules: oracle_step plus sparc_rules_oracle.c's audit of every env
after every step, pinned by the reference's golden rule_status bits."""
import functools

import numpy as np

from oracle import COracle, OraclePool, RulesCOracle
from oracle.cpu_ref import DIRS

# cell sizes, max_shaped of the random half, max_steps.  max_shaped=4 on C and D is a condition of
# the check: without it the random symbol soups hold regions whose exact-fit search (anchors^ylops,
# as in the reference) does not end in the oracle either
POOLS = {
    "A": (((3, 3),), None, 24),                                # 7x7: k_rollout1r, rows in LDS
    "B": (((2, 3), (3, 2), (2, 2), (1, 3)), None, 24),         # non-square boards, differing dims
    "C": (((2, 2), (3, 3), (4, 4), (5, 5)), 4, 60),            # multi-word boards: the generic kernel
    "D": (((7, 7), (6, 6)), 4, 60),                            # 13x13 / 15x15: memoised search, no table
}
_SEEDS = {"A": (41, 42), "B": (43, 44), "C": (45, 46), "D": (47, 48)}


@functools.lru_cache(maxsize=None)
def pool(name):
    """(processed puzzles, OraclePool, RulesCOracle) of pool `name`: 128 rule-consistent puzzles
    (a fraction broken) and 128 random full-property ones.  Built once per process; read only."""
    from sparc_gym_amd import synthetic
    from sparc_gym_amd.puzzles import process_puzzles
    sizes, max_shaped, _ = POOLS[name]
    s1, s2 = _SEEDS[name]
    recs = synthetic.make_rule_puzzles(128, seed=s1, sizes=sizes, break_prob=0.3)
    recs += synthetic.make_puzzles(128, seed=s2, sizes=sizes, full_properties=True, max_shaped=max_shaped)
    proc = process_puzzles(recs)
    return proc, OraclePool(step_pool(proc)), RulesCOracle(proc)


def step_pool(proc):
    return [{"x_size": p["x_size"], "y_size": p["y_size"], "start": list(p["start_location"]),
             "target": list(p["target_location"]), "solution_count": p["solution_count"],
             "solution_paths": p["solution_paths"], "gaps": p["obs_array"]["gaps"]} for p in proc]


def puzzle_indices(n, P):
    return (np.arange(n) * 37) % P


def _solution_actions(path):
    inv = {d: a for a, d in DIRS.items()}
    return [inv[(int(b[0]) - int(a[0]), int(b[1]) - int(a[1]))] for a, b in zip(path[:-1], path[1:])]


def actions(proc, pids, T, seed):
    """[T, n] uint8.  Random walks never solve a puzzle, so even envs start along a listed solution
    of their puzzle, solution_paths[(i // 2) % len]; every third of those is cut at a random point;
    after that, and in all odd envs, uniform 0..4 (4 is no action: the illegal-action path)."""
    rng = np.random.default_rng(seed)
    n = len(pids)
    acts = rng.integers(0, 5, size=(T, n)).astype(np.uint8)
    for i in range(0, n, 2):
        sols = proc[int(pids[i])]["solution_paths"]
        if not len(sols):
            continue
        plan = _solution_actions(sols[(i // 2) % len(sols)])
        if (i // 2) % 3 == 2:
            plan = plan[:int(rng.integers(len(plan) + 1))]
        plan = plan[:T]
        acts[:len(plan), i] = plan
    assert (acts == 4).any()
    return acts


def oracle_trace(name, n, T, traceback, autoreset, acts=None, seed=0, env_offset=0, max_steps=None):
    """The oracle's rollout of pool `name` over every env and step: dict with rew, flags, bits
    [T, n], stats [n, 4] and the final COracle.state()."""
    proc, opool, rules = pool(name)
    o = COracle(opool, n, traceback, POOLS[name][2] if max_steps is None else max_steps,
                autoreset={"none": 0, "next_step": 1}[autoreset])
    o.reset(puzzle_indices(n, len(proc)))
    stats = np.zeros((n, 4), np.int32)
    rew, flags, bits = o.rollout_rules(T, rules, acts, seed=seed, env_offset=env_offset, stats=stats)
    return {"rew": rew, "flags": flags, "bits": bits, "stats": stats, "state": o.state()}


def coverage(tr):
    """What an oracle trace exercises: counts of each rule bit set, done steps, bit patterns."""
    b = tr["bits"].astype(np.int64)
    return {"total": b.size, "minus1": int((b == -1).sum()),
            "set": [int(((b >> k) & 1).sum()) for k in range(10)],
            "done": int(((tr["flags"] & 3) != 0).sum()), "patterns": len(np.unique(b))}


def assert_coverage(name, tr, autoreset, drawn=False):
    """The floors of what a case must exercise, on the ORACLE's trace (a GPU output never feeds
    them).  Floors: about half of what the oracle gives with this recipe at 1,040 x 60 (520 x 60
    for D), see the counts in tests/test_gpu_rules_trace.py's docstring.  drawn: counter-hash
    random actions, no solution prefixes: the oracle gave the all-pass bit 38-84 times and
    reached_target 363-1,549 times, so those two floors are 15 and 150 there."""
    c = coverage(tr)
    assert c["minus1"] == 0, "the reference's KeyError case is not part of these pools"
    b = tr["bits"]
    # bits 1 and 2 (path_not_crossing, no_gap_violations): 1 in every state the env can reach, as
    # step() refuses moves onto visited points and gaps
    assert ((b & 6) == 6).all()
    assert c["set"][9] == 0
    if name in ("A", "B"):
        assert c["set"][8] >= (15 if drawn else 30), c
        for k in (0, 3, 4, 5, 6, 7):
            assert min(c["set"][k], c["total"] - c["set"][k]) >= (150 if drawn and k == 0 else 500), (k, c)
        if autoreset == "next_step":
            assert c["done"] >= 1000, c
        assert c["patterns"] >= 40, c
    else:
        assert c["set"][8] >= {"C": 20, "D": 3}[name], c
    return c
