"""The 64-bit counters of the counter-based RNG at values past 2^32, through every site that draws.

``seed``, ``t0``, ``env_offset`` and the playout ``id0`` are 64-bit in the ABI, and a long run gets
there: a cumulative ``t0`` passes 2^32 after minutes, ``env_offset + i`` does in a large sharded job.
The draw is written out separately in each rollout kernel, in k_rand_actions and in k_playout, so each
site is run here with

    seed = 0xF123456789ABCDEF, t0 = 2^32 - 5 (t0 + t carries at t = 5, inside the first 16-step tile),
    env_offset = 2^32 - 150 for 300 envs (env_offset + i carries at lane 22 of wave 2), 2^32 - 100
    otherwise (lane 36 of wave 1), and playouts with id0 = 2^63 + 2^32 - 700 over 1,500 ids,

bit-exact against the C oracle (reward codes, flags, stats, final state; planes and rule bits where
the kernel writes them).  A site that computed any of the three sums or products in 32 bits would
draw other actions: the guards below show that on the oracle's side alone, before any GPU result is
looked at: every reference here is computed behind its guard.  The guards need no GPU, and
tests/test_counters64_guards.py runs them as tests of their own in the run without one.

Left out: the slot path of k_rollout1s on a pool of more than 1,024 puzzles.  It is the same kernel
template with the same draw (RAND is independent of where the rows come from), and building
test_gpu_bigpool.py's 2,048-puzzle pool takes about six seconds on the host, several times what all
the cases here take together.

What the guard can ask of each variant: a seed without its upper half changes every entry, so every
64-env wave must differ; ``t0 + t`` wrapped changes the rows t >= 5 of every env, so every wave must
differ; ``env_offset + i`` wrapped changes only the envs at and after the carry (before it the sum is
below 2^32 and the wrap is the identity), so every wave that holds such an env must differ."""
import functools

import numpy as np
import pytest

import rules_trace as rt
from oracle import COracle
from sparc_gym_amd.search import rand_pick
from test_gpu_bigpool import _state_equal
from test_gpu_playout import _check_against, _host, _yardstick
from test_gpu_snapshot import MAX_STEPS, _copy_envs, _save_envs, _tables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 0xF123456789ABCDEF
T0 = 2**32 - 5
T = 35
ID0 = 2**63 + 2**32 - 700
K, L = 5, 6                       # 300 records x 5 playouts = 1,500 ids, the carry at id 700
M32, M64 = 2**32 - 1, 2**64 - 1
AUTORESET = {"none": 0, "next_step": 1}


def _off(n):
    return 2**32 - 150 if n == 300 else 2**32 - 100


def _pids(n, P):
    return (np.arange(n) * 7 + 3) % P


# ----------------------------------------------------------------------------- the draw in numpy
def _table(seed, env, t):
    """sparc_rand_action (include/sparc_gym_amd.h) for env ids [n] and steps [T] given as uint64
    arrays: [T, n] uint8."""
    u = lambda v: np.asarray([v & M64], np.uint64)  # noqa: E731
    env, t = np.asarray(env, np.uint64), np.asarray(t, np.uint64)
    with np.errstate(over="ignore"):
        z = u(seed)[None, :] + env[None, :] * u(0x9E3779B97F4A7C15) + t[:, None] * u(0xD1B54A32D192ED03)
        z = (z ^ (z >> np.uint64(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * u(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(62)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _tables64(n, T=T, t0=T0):
    """The action table of the full counters and of each 32-bit mistake, one at a time."""
    env = np.uint64(_off(n)) + np.arange(n, dtype=np.uint64)
    t = np.uint64(t0) + np.arange(T, dtype=np.uint64)
    out = {"full": _table(SEED, env, t), "seed32": _table(SEED & M32, env, t),
           "env32": _table(SEED, env & np.uint64(M32), t), "t32": _table(SEED, env, t & np.uint64(M32))}
    for a in out.values():
        a.setflags(write=False)
    return out


def _waves_that_differ(a, b):
    n = a.shape[1]
    col = (a != b).any(0)
    return np.array([col[w:w + 64].any() for w in range(0, n, 64)])


@functools.lru_cache(maxsize=None)
def _guard_table(n):
    """On the numpy draw and the oracle's own function: the table is the oracle's, and each 32-bit
    mistake changes it in every wave it can reach."""
    tabs = _tables64(n)
    o = COracle(_tables("7x7_full")[2], 1, True, MAX_STEPS)
    rng = np.random.default_rng(n)
    picks = [(t, i) for t in (0, 4, 5, 6, T - 1) for i in (0, 63, 64, n - 1)]
    picks += [(4, 2**32 - _off(n) - 1), (5, 2**32 - _off(n))]
    picks += list(zip(rng.integers(0, T, 200).tolist(), rng.integers(0, n, 200).tolist()))
    for t, i in picks:
        assert tabs["full"][t, i] == o.rand_action(SEED, _off(n) + i, T0 + t)
        assert tabs["seed32"][t, i] == o.rand_action(SEED & M32, _off(n) + i, T0 + t)
        assert tabs["env32"][t, i] == o.rand_action(SEED, (_off(n) + i) & M32, T0 + t)
        assert tabs["t32"][t, i] == o.rand_action(SEED, _off(n) + i, (T0 + t) & M32)
    assert set(np.unique(tabs["full"])) == {0, 1, 2, 3}
    assert _waves_that_differ(tabs["full"], tabs["seed32"]).all()
    assert _waves_that_differ(tabs["full"], tabs["t32"]).all()
    carry = 2**32 - _off(n)                                  # the first env whose id is past 2^32
    past = np.array([min(w + 64, n) > carry for w in range(0, n, 64)])
    assert 0 < carry < n and carry % 64 and past.sum() >= 3
    assert np.array_equal(_waves_that_differ(tabs["full"], tabs["env32"]), past)
    assert np.array_equal(tabs["full"][:5], tabs["t32"][:5]) and (tabs["full"][5:] != tabs["t32"][5:]).any(1).all()
    return True


@functools.lru_cache(maxsize=None)
def _ref(name, tb, n, autoreset, obs=False):
    """The oracle's run of the drawn actions at the large counters (computed once, read only), after
    the guard: the oracle drew exactly the numpy table, and under each 32-bit mistake its reward
    codes come out different."""
    _guard_table(n)
    proc, table, pool = _tables(name)
    pids = _pids(n, len(proc))

    def run(acts, planes=False):
        o = COracle(pool, n, tb, MAX_STEPS, autoreset=AUTORESET[autoreset])
        o.reset(pids)
        st = np.zeros((n, 4), np.int32)
        if planes:
            out = o.rollout_obs(T, table.x_max, table.y_max, acts, seed=SEED, env_offset=_off(n), t0=T0, stats=st)
        else:
            out = o.rollout(T, acts, seed=SEED, env_offset=_off(n), t0=T0, stats=st)
        return out, st, o

    tabs = _tables64(n)
    out, st, o = run(None, obs)
    given, st_given, _ = run(tabs["full"])
    assert np.array_equal(out[0], given[0]) and np.array_equal(out[1], given[1]) and np.array_equal(st, st_given)
    for k in ("seed32", "env32", "t32"):
        wrong, _, _ = run(tabs[k])
        assert not np.array_equal(wrong[0], out[0]), f"reward codes blind to {k}"
        assert _waves_that_differ(wrong[0], out[0]).sum() >= 3, k
    assert (out[1] & 3).any() and ((out[1] & 64) != 0).any() == (autoreset == "next_step")
    ref = dict(rew=out[0], flags=out[1], stats=st, state=o.state(), pids=pids, proc=proc, table=table)
    if obs:
        ref.update(visited=out[2], agent=out[3])
    return ref


# ----------------------------------------------------------------------------- the playout ids
def _pick_ids(MK=300 * K):
    return np.uint64(ID0) + np.arange(MK, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _guard_picks():
    """search.rand_pick (pinned against the C function by test_rand_pick.py) over the playout ids: an
    id or a seed cut to 32 bits draws differently in every wave of 64 playouts the cut can reach."""
    ids, t = _pick_ids(), np.arange(L, dtype=np.uint64)[:, None]
    full = rand_pick(SEED, ids[None, :], t, 15)
    assert _waves_that_differ(full, rand_pick(SEED & M32, ids[None, :], t, 15)).all()
    cut = _waves_that_differ(full, rand_pick(SEED, ids[None, :] & np.uint64(M32), t, 15))
    assert cut.all()                                         # bit 63 of id0 is lost in every id
    assert int(ids[699]) & M32 == M32 and int(ids[700]) & M32 == 0
    g = np.arange(len(ids))
    lost = np.where(g >= 700, ids - np.uint64(2**32), ids)   # a carry into bit 32 that is dropped
    past = np.array([min(w + 64, len(ids)) > 700 for w in range(0, len(ids), 64)])
    assert np.array_equal(_waves_that_differ(full, rand_pick(SEED, lost[None, :], t, 15)), past) and past.sum() > 12
    return True


# ----------------------------------------------------------------------------- the rollout kernels
def _vec(ref, tb, n, autoreset, **kw):
    from sparc_gym_amd import SPaRCVecEnv
    args = dict(processed=ref["proc"], table=ref["table"], traceback=tb, max_steps=MAX_STEPS, autoreset=autoreset,
                observation="compact", env_offset=_off(n))
    args.update(kw)
    v = SPaRCVecEnv(n, **args)
    v.reset(options={"puzzle_index": ref["pids"]})
    return v


def _same_run(v, out, stats, ref):
    assert np.array_equal(out["reward_code"].cpu().numpy(), ref["rew"]), "reward codes"
    assert np.array_equal(out["flags"].cpu().numpy(), ref["flags"]), "flags"
    assert np.array_equal(stats.cpu().numpy(), ref["stats"]), "stats"
    _state_equal(v.state(), ref["state"], v.table)


# kernel the case reaches (sparc_kernels.hip, rollout_impl): name, traceback, n, autoreset
ROLLOUTS = [
    pytest.param("7x7_full", True, 272, "next_step", id="k_rollout1-tiled-n272"),
    pytest.param("7x7_full", True, 300, "next_step", id="k_rollout1-untiled-n300"),
    pytest.param("7x7_full", True, 256, "next_step", id="k_rollout1s-tb-ior"),
    pytest.param("7x7_full", False, 256, "next_step", id="k_rollout1s-notb-ior"),
    pytest.param("7x7_full", True, 256, "none", id="k_rollout1s-tb-noior"),
    pytest.param("7x7_full", False, 256, "none", id="k_rollout1s-notb-noior"),
    pytest.param("mixed_5_11", True, 256, "next_step", id="k_rolloutWs-W2"),
    pytest.param("15x15", True, 256, "next_step", id="k_rolloutWs-W4"),
    pytest.param("15x15", False, 256, "none", id="k_rolloutWs-W4-noior"),
    pytest.param("mixed_5_11", True, 300, "next_step", id="k_rollout-W2-n300"),
    pytest.param("mixed_5_11", False, 272, "next_step", id="k_rollout-W2-tiled-n272"),
]


@pytest.mark.parametrize("name,tb,n,autoreset", ROLLOUTS)
def test_drawn_rollout_at_large_counters(on_gpu, name, tb, n, autoreset):
    """T = 35: on 256 envs the split kernels run the first 32 steps and the per-wave kernel the last
    three (t0 advanced by 32 between the launches); other batch sizes run the per-wave kernel alone."""
    ref = _ref(name, tb, n, autoreset)
    v = _vec(ref, tb, n, autoreset)
    stats = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    out = v.rollout(T, None, seed=SEED, t0=T0, stats=stats)
    _same_run(v, out, stats, ref)


@pytest.mark.parametrize("name,tb,n", [("7x7_full", True, 256), ("mixed_5_11", True, 256), ("mixed_5_11", False, 300)])
def test_chunked_run_equals_one_launch_across_the_carry(on_gpu, name, tb, n):
    ref = _ref(name, tb, n, "next_step")
    v = _vec(ref, tb, n, "next_step")
    stats = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    a = v.rollout(20, None, seed=SEED, t0=T0, stats=stats)
    b = v.rollout(15, None, seed=SEED, t0=T0 + 20, stats=stats)
    out = {k: torch.cat([a[k], b[k]]) for k in ("reward_code", "flags")}
    _same_run(v, out, stats, ref)


@pytest.mark.parametrize("name,tb,n", [("7x7_full", True, 256), ("7x7_full", False, 300), ("mixed_5_11", True, 300)])
def test_random_actions_are_the_oracle_table_and_what_the_rollout_drew(on_gpu, name, tb, n):
    ref = _ref(name, tb, n, "next_step")
    v = _vec(ref, tb, n, "next_step")
    acts = v.random_actions(T, seed=SEED, t0=T0)
    assert np.array_equal(acts.cpu().numpy(), _tables64(n)["full"])
    stats = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    out = v.rollout(T, acts, stats=stats)                     # given: the drawn rollout's actions
    _same_run(v, out, stats, ref)


@pytest.mark.parametrize("inline", [False, True], ids=["k_rollout_obsw", "k_rollout-obs-inline"])
@pytest.mark.parametrize("name,n", [("mixed_5_11", 300), ("7x7_full", 272)])
def test_drawn_observation_rollout_at_large_counters(on_gpu, name, n, inline):
    ref = _ref(name, True, n, "next_step", True)
    v = _vec(ref, True, n, "next_step", observation="new")
    if inline:
        v.core.set_variant(v.core.VARIANT_OBS_INLINE, 1)
    stats = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    out = v.rollout(T, None, seed=SEED, t0=T0, stats=stats, obs=True)
    assert np.array_equal(out["visited"].cpu().numpy(), ref["visited"])
    assert np.array_equal(out["agent_location"].cpu().numpy(), ref["agent"])
    _same_run(v, out, stats, ref)


# ----------------------------------------------------------------------------- the rule rollouts
@functools.lru_cache(maxsize=None)
def _rules_ref(pool, n):
    _guard_table(n)
    proc, opool, rules = rt.pool(pool)
    pids = rt.puzzle_indices(n, len(proc))

    def run(acts):
        o = COracle(opool, n, False, rt.POOLS[pool][2], autoreset=1)
        o.reset(pids)
        st = np.zeros((n, 4), np.int32)
        return o.rollout_rules(T, rules, acts, seed=SEED, env_offset=_off(n), t0=T0, stats=st), st, o

    (rew, flags, bits), st, o = run(None)
    for k in ("seed32", "env32", "t32"):
        (r2, _, b2), _, _ = run(_tables64(n)[k])
        assert not np.array_equal(r2, rew) and not np.array_equal(b2, bits), f"rule rollout blind to {k}"
    assert (bits >= 0).all() and len(np.unique(bits)) >= 8
    return dict(rew=rew, flags=flags, bits=bits, stats=st, state=o.state(), pids=pids, proc=proc)


@pytest.mark.parametrize("pool,words,variant", [("A", 1, ("VARIANT_R1R_SHAPE", 0)), ("A", 1, ("VARIANT_R1R_SHAPE", 1)),
                                                ("A", 1, ("VARIANT_RULE_ROLLOUT_GENERIC", 1)),
                                                ("C", 2, ("VARIANT_RULE_ROLLOUT_GENERIC", 1))],
                         ids=["k_rollout1r-shape0", "k_rollout1r-shape1", "k_rollout-rules-W1", "k_rollout-rules-W2"])
def test_drawn_rule_rollout_at_large_counters(on_gpu, pool, words, variant):
    from sparc_gym_amd import SPaRCVecEnv
    n = 300
    ref = _rules_ref(pool, n)
    v = SPaRCVecEnv(n, processed=ref["proc"], traceback=False, autoreset="next_step", observation="compact",
                    rules=True, max_steps=rt.POOLS[pool][2], env_offset=_off(n))
    assert v.table.words == words
    v.core.set_variant(getattr(v.core, variant[0]), variant[1])
    v.reset(options={"puzzle_index": ref["pids"]})
    stats = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    out = v.rollout(T, None, seed=SEED, t0=T0, stats=stats, rules=True)
    assert np.array_equal(out["rule_bits"].cpu().numpy(), ref["bits"]), "rule bits"
    _same_run(v, out, stats, ref)


# ----------------------------------------------------------------------------- the playout draw
@pytest.mark.parametrize("name,tb,forward", [("7x7_full", True, True), ("mixed_5_11", False, False),
                                             ("15x15", True, False)])
def test_playout_at_large_seed_and_ids(on_gpu, name, tb, forward):
    """k_playout's uint_rand_pick with ids id0 + g that cross 2^32 at g = 700 and have bit 63 set:
    against the chained-expand yardstick (ids summed in uint64) and the oracle's replay of the trace."""
    n = 300
    assert _guard_picks()
    ref = _ref(name, tb, n, "next_step")
    v = _vec(ref, tb, n, "next_step")
    v.rollout(T, None, seed=SEED, t0=T0)                      # the roots: the oracle's final state
    _state_equal(v.state(), ref["state"], v.table)
    snap = v.snapshot()
    out = v.playout(snap, K, L, seed=SEED, id0=ID0, forward_only=forward, trace=True, final=True)
    _check_against(out, _yardstick(v, snap, K, L, SEED, ID0, forward), n, K, L)
    got = _host(out)
    MK = n * K
    trace, steps = got["trace"].reshape(L, MK), got["steps"].reshape(MK).astype(np.int64)
    code, flags = got["reward_code"].reshape(MK), got["flags"].reshape(MK)
    assert (steps > 0).sum() > MK // 2
    proc, _, pool = _tables(name)
    src = COracle(pool, n, tb, MAX_STEPS, autoreset=1)         # the same run again: its structs are the roots
    src.reset(ref["pids"])
    src.rollout(T, None, seed=SEED, env_offset=_off(n), t0=T0)
    saved = _save_envs(src)
    o = COracle(pool, MK, tb, MAX_STEPS, autoreset=0)
    _copy_envs(o, saved, np.arange(MK) // K)
    for t in range(L):
        legal = np.array([o.legal(i) for i in range(MK)], np.int64)
        stepped = trace[t] != 255
        assert ((legal >> np.minimum(trace[t], 3)) & 1 != 0)[stepped & (legal != 0)].all()
        r, f = o.rollout(1, trace[t][None])
        last = stepped & (steps == t + 1)
        assert np.array_equal(r[0][last], code[last]) and np.array_equal(f[0][last], flags[last])
    v.core.sync()
