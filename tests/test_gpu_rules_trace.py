"""The rule bits of EVERY env after EVERY step of a rule rollout against the C oracle
(COracle.rollout_rules: oracle_step + sparc_rules_oracle.c's audit, pinned by the reference's golden
rule_status bits), on every kernel that produces them: k_rollout1r in each compiled shape, the
generic k_rollout<..., RULES>, with traceback on and off, next-step autoreset and none, actions
given or drawn on the device; and k_rules and the record audits (generic and table-only) on the
final state of every env.  No sampling: each case compares n x (T1 + T2) audits, two launches on
one context so the state crosses HBM mid-episode, T1 = 37 and T2 = 23 so that every launch ends in
a ragged tile for the tile lengths 15, 12, 10 and 4.

Pools, action streams and the floors of what a case must exercise are in tests/rules_trace.py; the
floors are asserted on the oracle's trace alone.  What the oracle gave with this recipe (counts of
n x 60 audits; ranges over traceback x autoreset):

  pool A, 1,040 envs, given actions: all-pass bit 64-299, reached_target 616-3,343, bits 3-7
      8,200-49,586 set, 2,359+ done steps, 58-60 bit patterns;
  pool A, drawn actions: all-pass 39-84, reached_target 379-1,549, 2,274+ done steps, 56-62 patterns;
  pool B: all-pass 123-585, reached_target 897-4,707, 58-60 patterns;
  pool C: all-pass 52-303, 58-60 patterns;  pool D (520 envs): all-pass 7-40, 47-48 patterns.
"""
import functools

import numpy as np
import pytest

import rules_trace as rt

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T1, T2 = 37, 23
SEED, ENV_OFFSET = 7, 12345


def _case(pool, tb, autoreset="next_step", given=True, n=1040, shape=0, generic=False, limits=None, unaligned=False,
          tag=None):
    c = dict(pool=pool, tb=tb, autoreset=autoreset, given=given, n=n, shape=shape, generic=generic,
             limits=limits or {}, unaligned=unaligned)
    cid = f"{pool}-traceback={tb}-autoreset={autoreset}-{'given' if given else f'drawn_env_offset={ENV_OFFSET}'}"
    return pytest.param(c, id=cid + (f"-{tag}" if tag else ""))


CASES = [_case("A", tb, ar, given) for tb in (False, True) for ar in ("next_step", "none") for given in (True, False)]
CASES += [_case("A", False, shape=s, tag=f"r1r_shape={s}") for s in (1, 2, 3, 4, 5)]
CASES += [_case("A", tb, generic=True, tag="generic_kernel") for tb in (False, True)]
CASES += [_case("A", False, limits=dict(rule_table_entries=40 * 512, fit_cap=1), tag="table_and_search"),
          _case("A", False, n=1000, tag="n=1000_untiled"),
          _case("A", True, unaligned=True, tag="unaligned_actions")]
CASES += [_case("B", tb) for tb in (False, True)]
CASES += [_case("C", tb, ar) for tb in (False, True) for ar in ("next_step", "none")]
CASES += [_case("D", tb, n=520) for tb in (False, True)]


@functools.lru_cache(maxsize=None)
def _given_actions(pool, n):
    proc, _, _ = rt.pool(pool)
    a = rt.actions(proc, rt.puzzle_indices(n, len(proc)), T1 + T2, seed=5)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _oracle(pool, n, tb, autoreset, given):
    """The oracle's trace of a case, computed once and shared by the cases that differ only in the
    kernel; read only."""
    tr = rt.oracle_trace(pool, n, T1 + T2, tb, autoreset, _given_actions(pool, n) if given else None,
                         seed=SEED, env_offset=ENV_OFFSET)
    for v in list(tr.values()) + list(tr["state"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    rt.assert_coverage(pool, tr, autoreset, drawn=not given)
    return tr


def _same(got, want, what, c):
    if not np.array_equal(got, want):
        bad = np.argwhere(np.asarray(got) != np.asarray(want))
        k = tuple(int(x) for x in bad[0])
        raise AssertionError(f"{what} differs at {len(bad)} of {np.asarray(want).size} places, first at "
                             f"(step, env) or (env, ...) = {k}: got {np.asarray(got)[k]}, oracle {np.asarray(want)[k]}; case {c}")


@pytest.mark.parametrize("c", CASES)
def test_rule_rollout_every_env_every_step(on_gpu, c):
    from sparc_gym_amd import SPaRCVecEnv
    from sparc_gym_amd.core import visited_planes
    proc, _, _ = rt.pool(c["pool"])
    n, T = c["n"], T1 + T2
    want = _oracle(c["pool"], n, c["tb"], c["autoreset"], c["given"])
    vec = SPaRCVecEnv(n, processed=proc, traceback=c["tb"], autoreset=c["autoreset"], observation="compact",
                      rules=True, max_steps=rt.POOLS[c["pool"]][2], env_offset=0 if c["given"] else ENV_OFFSET,
                      **c["limits"])
    if c["shape"]:
        vec.core.set_variant(vec.core.VARIANT_R1R_SHAPE, c["shape"])
    if c["generic"]:
        vec.core.set_variant(vec.core.VARIANT_RULE_ROLLOUT_GENERIC, 1)
    vec.reset(options={"puzzle_index": rt.puzzle_indices(n, len(proc))})
    a1 = a2 = None
    if c["given"]:
        host = torch.from_numpy(_given_actions(c["pool"], n).copy())
        if c["unaligned"]:   # both launches' action pointers 1 past a 16-byte boundary: no tiled I/O
            buf = torch.empty(T * n + 16, dtype=torch.uint8, device="cuda")
            acts = buf[1:1 + T * n].view(T, n)
            acts.copy_(host)
            assert acts.data_ptr() % 16 == 1 and acts[T1:].data_ptr() % 16 == 1 and acts.is_contiguous()
        else:
            acts = host.cuda()
            assert acts.data_ptr() % 16 == 0
        a1, a2 = acts[:T1], acts[T1:]
    stats = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    r1 = vec.rollout(T1, a1, seed=SEED, t0=0, stats=stats, rules=True)
    r2 = vec.rollout(T2, a2, seed=SEED, t0=T1, stats=stats, rules=True)
    rew, flags, bits = (torch.cat([r1[k], r2[k]]).cpu().numpy() for k in ("reward_code", "flags", "rule_bits"))
    assert bits.shape == (T, n) and bits.dtype == np.int16
    assert not (bits & (1 << 9)).any()   # no exact-fit search left unfinished
    _same(bits, want["bits"], "rule bits", c)
    _same(rew, want["rew"], "reward codes", c)
    _same(flags, want["flags"], "flags", c)
    _same(stats.cpu().numpy(), want["stats"], "stats", c)
    s, so = vec.state(), want["state"]
    for k, ko in (("x", "x"), ("y", "y"), ("step", "step"), ("path_len", "path_len"), ("puzzle", "pid"),
                  ("outcome", "outcome")):
        _same(s[k].astype(np.int64), so[ko], k, c)
    _same(visited_planes(s["visited"], vec.table, 16, 16), so["visited"].astype(np.int32), "visited", c)
    # k_rules and the record audit on the state the rollouts left: the oracle's last-step bits
    _same(vec.rule_audit()["bits"].cpu().numpy(), want["bits"][-1], "rule_audit() bits", c)
    _same(vec.audit_records(vec.snapshot())["bits"].cpu().numpy(), want["bits"][-1], "audit_records() bits", c)
