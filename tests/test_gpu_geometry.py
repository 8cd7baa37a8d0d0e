"""Every kernel family on every board geometry the packer can choose (tests/geometry_pools.py).

Every kernel indexes a board as bit x * pitch + y of a `words`-word bitboard; the standing pools
of the suite run pitch 8 on one word, 9 and 11 on two, 15 and 16 on four.  Here the other thirteen
(words, pitch) classes of the default packing run, and three pools (3x3, 5x5, 7x7) under forced
geometries, whose results must not depend on the geometry.  Every comparison is bit-exact against
the C oracle (COracle, RulesCOracle), or against oracle/rules_ref.py, tests/dfs_ref.py and
tests/record_path.py where the C oracle has no entry; the oracle's traces are computed once per
pool (the classes of a family share them) and are read only.

Shapes, the smallest that reach each kernel: n = 512 (two full 256-env workgroups: the split
kernels run) and n = 300 (a partial workgroup: the whole launch goes through k_rollout1 /
k_rollout); T = 53 (three 16-step tiles through the split kernel, then a 5-step tail through the
non-split kernel, in one call); max_steps 24 (truncations and autoresets inside the launch); 64
puzzles.  Actions are rules_trace.actions: solution prefixes on even envs, uniform 0..4 elsewhere.

The coverage floors (truncated, +100, -100, autoreset, pop, illegal action, all-pass state) are
asserted on the ORACLE's trace alone; the floors and the oracle's counts are in
tests/geometry_pools.py (FLOORS)."""
import ctypes
import functools

import numpy as np
import pytest

import geometry_pools as gp
import record_path
from oracle import COracle, _Env, rules_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T, T_RULES, T_OBS = 53, 48, 20
NS = (512, 300)
MODES = ("next_step", "none")
ALL = list(gp.CLASSES)
SNAP = gp.SNAP_STEP


# ----------------------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def _rules_table(name):
    from sparc_gym_amd.puzzles import pack_rules
    proc, table = gp.rule_pool(name)[:2]
    return pack_rules(proc, table)


def _vec(name, n, tb, autoreset="next_step", rule=False, observation="compact", **kw):
    from sparc_gym_amd import SPaRCVecEnv
    proc, table = (gp.rule_pool if rule else gp.step_pool)(name)[:2]
    v = SPaRCVecEnv(n, processed=proc, table=table, traceback=tb, max_steps=gp.MAX_STEPS, autoreset=autoreset,
                    observation=observation, **kw)
    if rule:   # SPaRCVecEnv(rules=True) with the class's rule table packed once, not once per context
        v.core.load_rules(_rules_table(name))
        v._rbits = torch.empty(n, dtype=torch.int16, device="cuda")
        v.rules = True
    return v


def _pids(name, n, rule=False):
    return gp.puzzle_indices(n, len((gp.rule_pool if rule else gp.step_pool)(name)[0]))


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()     # a copy: the cached arrays are read only


def _same(got, want, what, case):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or not np.array_equal(got, want):
        assert got.shape == want.shape, f"{what}: shape {got.shape}, oracle {want.shape}; case {case}"
        bad = np.argwhere(got != want)
        k = tuple(int(x) for x in bad[0])
        raise AssertionError(f"{what} differs at {len(bad)} of {want.size} places, first at {k}: got {got[k]}, "
                             f"oracle {want[k]}; case {case}")


def _state_same(s, so, table, case):
    """Positions and boards decoded through the table, against the oracle's state."""
    from sparc_gym_amd.core import visited_planes
    for k, ko in (("x", "x"), ("y", "y"), ("step", "step"), ("path_len", "path_len"), ("puzzle", "pid"),
                  ("outcome", "outcome")):
        _same(np.asarray(s[k]).astype(np.int64), so[ko], k, case)
    planes = visited_planes(s["visited"], table, 16, 16)
    _same(planes, so["visited"].astype(np.int32), "visited planes", case)
    _same(gp.decode_board(s["visited"], table), so["visited"].astype(np.int32), "visited bits x * pitch + y", case)


def _rollout(name, n, tb, autoreset, io_off=False):
    """One rollout(T, actions) launch on a fresh context: codes, flags, stats, state."""
    v = _vec(name, n, tb, autoreset)
    if io_off:
        v.core.set_variant(v.core.VARIANT_IO_CODES_OFF, 1)
    v.reset(options={"puzzle_index": _pids(name, n)})
    stats = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    out = v.rollout(T, _dev(gp.actions(name, n, T)), stats=stats)
    return out["reward_code"].cpu().numpy(), out["flags"].cpu().numpy(), stats.cpu().numpy(), v.state()


# ----------------------------------------------------------------------------- (a) step and rollout
@pytest.mark.parametrize("tb", [True, False])
@pytest.mark.parametrize("name", ALL)
def test_rollout_step_oracle_agree(on_gpu, name, tb):
    """rollout(T, actions) in one launch, T step() calls and the oracle: reward codes, flags, stats
    and the final state (x, y, step, path_len, puzzle, outcome, visited planes), for both autoreset
    modes and both n."""
    table = gp.step_pool(name)[1]
    for autoreset in MODES:
        for n in NS:
            case = (name, tb, autoreset, n)
            want = gp.step_trace(name, n, T, tb, autoreset)
            gp.assert_step_coverage(name, want, tb, autoreset)
            ra, fa, sa, state_a = _rollout(name, n, tb, autoreset)
            _same(ra, want["rew"], "rollout reward codes", case)
            _same(fa, want["flags"], "rollout flags", case)
            _same(sa, want["stats"], "rollout stats", case)
            _state_same(state_a, want["state"], table, case)
            b = _vec(name, n, tb, autoreset)
            b.reset(options={"puzzle_index": _pids(name, n)})
            acts = _dev(gp.actions(name, n, T))
            rb = torch.empty((T, n), dtype=torch.int8, device="cuda")
            fb = torch.empty((T, n), dtype=torch.uint8, device="cuda")
            for t in range(T):
                _, _, _, _, info = b.step(acts[t])
                rb[t], fb[t] = info["reward_code"], b._flags
            _same(rb.cpu().numpy(), want["rew"], "step() reward codes", case)
            _same(fb.cpu().numpy(), want["flags"], "step() flags", case)
            _state_same(b.state(), want["state"], table, case)


@pytest.mark.parametrize("name", ALL)
def test_drawn_rollout_and_io_codes_off(on_gpu, name):
    """Actions drawn on the device (seed, t0, env_offset) against the oracle's restatement of the
    hash; and SPARC_VARIANT_IO_CODES_OFF (the split rollouts keep the reward codes on the trie wave):
    its outputs equal the default's and the oracle's."""
    proc, table, opool = gp.step_pool(name)
    n, seed, t0, off = 512, 99, 7, 12345
    for tb in (True, False):
        v = _vec(name, n, tb, env_offset=off)
        v.reset(options={"puzzle_index": _pids(name, n)})
        stats = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        out = v.rollout(T, None, seed=seed, t0=t0, stats=stats)
        o = COracle(opool, n, tb, gp.MAX_STEPS, autoreset=1)
        o.reset(_pids(name, n))
        ost = np.zeros((n, 4), np.int32)
        ro, fo = o.rollout(T, None, seed=seed, env_offset=off, t0=t0, stats=ost)
        case = (name, tb, "drawn")
        _same(out["reward_code"].cpu().numpy(), ro, "reward codes", case)
        _same(out["flags"].cpu().numpy(), fo, "flags", case)
        _same(stats.cpu().numpy(), ost, "stats", case)
        _state_same(v.state(), o.state(), table, case)
        want = gp.step_trace(name, n, T, tb, "next_step")
        r0, f0, s0, st0 = _rollout(name, n, tb, "next_step")
        r1, f1, s1, st1 = _rollout(name, n, tb, "next_step", io_off=True)
        case = (name, tb, "io_codes_off")
        for got, dflt, key in ((r1, r0, "rew"), (f1, f0, "flags"), (s1, s0, "stats")):
            _same(got, dflt, key + " vs the default", case)
            _same(got, want[key], key, case)
        _state_same(st1, want["state"], table, case)


# ----------------------------------------------------------------------------- (b) other geometry
@pytest.mark.parametrize("family", list(gp.FAMILIES))
def test_same_puzzles_under_every_geometry(on_gpu, family):
    """One pool packed at several pitches and widths: codes, flags, stats and the decoded final
    state are identical across the geometries and equal to the oracle's."""
    from sparc_gym_amd.core import visited_planes
    names = gp.FAMILIES[family]
    assert len({gp.CLASSES[k]["geom"][:2] for k in names}) == len(names) >= 3
    for tb in (True, False):
        for n in NS:
            want = gp.step_trace(names[0], n, T, tb, "next_step")
            first = None
            for name in names:
                assert gp.step_trace(name, n, T, tb, "next_step") is want      # one oracle trace per family
                table = gp.step_pool(name)[1]
                r, f, s, st = _rollout(name, n, tb, "next_step")
                got = [r, f, s] + [np.asarray(st[k]).astype(np.int64) for k in ("x", "y", "step", "path_len", "puzzle",
                                                                                 "outcome")]
                got.append(visited_planes(st["visited"], table, 16, 16))
                if first is None:
                    first = got
                    _same(r, want["rew"], "reward codes", (name, tb, n))
                    _same(f, want["flags"], "flags", (name, tb, n))
                    _state_same(st, want["state"], table, (name, tb, n))
                for a, b in zip(got, first):
                    _same(a, b, f"{name} vs {names[0]}", (family, tb, n))


# ----------------------------------------------------------------------------- (c) rows from the L2
@pytest.fixture(scope="module")
def big_w1p6():
    from sparc_gym_amd import synthetic
    from sparc_gym_amd.puzzles import pack_table, process_puzzles
    recs = synthetic.make_puzzles(2048, seed=5, sizes=gp.CLASSES["w1p6"]["sizes"], n_solutions=8,
                                  shared_prefix_prob=0.9, full_properties=True)
    proc = process_puzzles(recs)
    table = pack_table(proc)
    assert (table.words, table.pitch, table.x_max, table.y_max) == gp.CLASSES["w1p6"]["geom"]
    return proc, table, gp.OraclePool(gp.oracle_puzzles(proc))


@pytest.mark.parametrize("max_steps", [2, 24])
@pytest.mark.parametrize("mixed", [0, 1])
def test_rows_from_the_l2_at_pitch_6(on_gpu, big_w1p6, mixed, max_steps):
    """A 2,048-puzzle pool past the LDS row budget at pitch 6: k_rollout1s reads the rows from the
    L2 (the row slots; max_steps 2 makes the slot rule fall back), with the 8-B trie records and
    with the mixed trie tables (SPARC_VARIANT_MIXED_TRIE), traceback on and off."""
    from sparc_gym_amd import SPaRCVecEnv
    proc, table, opool = big_w1p6
    n = 512
    for tb in (True, False):
        rng = np.random.default_rng(max_steps + 100 * tb)
        pids = rng.integers(len(proc), size=n)
        acts = rng.integers(0, 4, size=(T, n)).astype(np.uint8)
        v = SPaRCVecEnv(n, processed=proc, table=table, traceback=tb, max_steps=max_steps, observation="compact")
        v.core.set_variant(v.core.VARIANT_MIXED_TRIE, mixed)
        v.reset(options={"puzzle_index": pids})
        st = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        out = v.rollout(T, _dev(acts), stats=st)
        o = COracle(opool, n, tb, max_steps, autoreset=1)
        o.reset(pids)
        ost = np.zeros((n, 4), np.int32)
        ro, fo = o.rollout(T, acts, stats=ost)
        case = (mixed, max_steps, tb)
        _same(out["reward_code"].cpu().numpy(), ro, "reward codes", case)
        _same(out["flags"].cpu().numpy(), fo, "flags", case)
        _same(st.cpu().numpy(), ost, "stats", case)
        _state_same(v.state(), o.state(), table, case)
        assert ost[:, 3].sum() > n                                # autoresets inside the launch
        assert max_steps < 24 or (ro == 100).any()                # and solved episodes


# ----------------------------------------------------------------------------- (d) observations
def _plane_dims(table):
    X, Y = table.x_max, table.y_max
    dims = [(X, Y), (X + 1, Y)]
    if X * (Y + 1) <= 256:
        dims.append((X, Y + 1))          # y_dim != pitch: the LUT path on multi-word pools too
    assert all(x * y <= 256 for x, y in dims)
    return dims


@functools.lru_cache(maxsize=6)
def _oracle_obs(name, tb, xd, yd):
    """The oracle's codes, flags and planes of a pool (name: gp.canonical); the classes of a family
    run one after the other, so the few entries kept are the family's."""
    n = 300
    proc, _, opool = gp.step_pool(name)
    o = COracle(opool, n, tb, gp.MAX_STEPS, autoreset=1)
    o.reset(gp.puzzle_indices(n, len(proc)))
    return o.rollout_obs(T_OBS, xd, yd, gp.actions(name, n, T)[:T_OBS])


def _obs_vec(name, n, tb, xd, yd):
    v = _vec(name, n, tb, observation="new")
    v.x_dim, v.y_dim = xd, yd
    v._vis = torch.empty((n, xd, yd), dtype=torch.int32, device="cuda")     # reset() packs into these
    v._agent = torch.empty_like(v._vis)
    v.reset(options={"puzzle_index": _pids(name, n)})
    return v


@pytest.mark.parametrize("tb", [True, False])
@pytest.mark.parametrize("name", ALL)
def test_observation_planes_every_env_every_step(on_gpu, name, tb):
    """rollout(obs=True) with the writer waves, the inline variant, and step(): the visited and
    agent_location planes of every env after every step against the oracle's, at plane sizes
    (x_max, y_max), (x_max + 1, y_max) and (x_max, y_max + 1)."""
    n = 300
    table = gp.step_pool(name)[1]
    acts = _dev(gp.actions(name, n, T)[:T_OBS])
    for xd, yd in _plane_dims(table):
        ro, fo, vo, ao = _oracle_obs(gp.canonical(name), tb, xd, yd)
        assert vo.any(axis=(0, 1)).sum() > 1 and ((fo & 64) != 0).any()
        vo_d, ao_d = _dev(vo), _dev(ao)
        for inline in (False, True):
            case = (name, tb, xd, yd, "inline" if inline else "writer waves")
            v = _obs_vec(name, n, tb, xd, yd)
            if inline:
                v.core.set_variant(v.core.VARIANT_OBS_INLINE, 1)
            out = v.rollout(T_OBS, acts, obs=True)
            _same(out["reward_code"].cpu().numpy(), ro, "reward codes", case)
            _same(out["flags"].cpu().numpy(), fo, "flags", case)
            if not torch.equal(out["visited"], vo_d):
                _same(out["visited"].cpu().numpy(), vo, "visited planes", case)
            if not torch.equal(out["agent_location"], ao_d):
                _same(out["agent_location"].cpu().numpy(), ao, "agent planes", case)
        b = _obs_vec(name, n, tb, xd, yd)
        for t in range(T_OBS):
            obs, _, _, _, info = b.step(acts[t])
            case = (name, tb, xd, yd, "step", t)
            if not (torch.equal(obs["visited"], vo_d[t]) and torch.equal(obs["agent_location"], ao_d[t])):
                _same(obs["visited"].cpu().numpy(), vo[t], "visited planes", case)
                _same(obs["agent_location"].cpu().numpy(), ao[t], "agent planes", case)
            if not torch.equal(info["reward_code"], _dev(ro[t])):
                _same(info["reward_code"].cpu().numpy(), ro[t], "reward codes", case)


# ----------------------------------------------------------------------------- (e) rule audit
@pytest.mark.parametrize("tb", [True, False])
@pytest.mark.parametrize("name", ALL)
def test_rule_rollout_every_env_every_step(on_gpu, name, tb):
    """rollout(rules=True) over every env and every step against COracle.rollout_rules, both
    autoreset modes and both n; on one-word ring_ok pools (k_rollout1r) again on the generic kernel
    (SPARC_VARIANT_RULE_ROLLOUT_GENERIC).  k_rules and the record audit on the state the rollout
    left give the oracle's last-step bits."""
    table = gp.rule_pool(name)[1]
    for autoreset in MODES:
        for n in NS:
            want = gp.rule_trace(name, n, T_RULES, tb, autoreset)
            gp.assert_rule_coverage(name, want)
            acts = _dev(gp.actions(name, n, T_RULES, rule=True))
            for generic in ((False, True) if gp.CLASSES[name]["ring_ok"] == 1 else (False,)):
                case = (name, tb, autoreset, n, "generic" if generic else "default")
                vec = _vec(name, n, tb, autoreset, rule=True)
                if generic:
                    vec.core.set_variant(vec.core.VARIANT_RULE_ROLLOUT_GENERIC, 1)
                vec.reset(options={"puzzle_index": _pids(name, n, rule=True)})
                stats = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
                out = vec.rollout(T_RULES, acts, stats=stats, rules=True)
                bits = out["rule_bits"].cpu().numpy()
                assert bits.shape == (T_RULES, n) and bits.dtype == np.int16
                _same(bits, want["bits"], "rule bits", case)
                _same(out["reward_code"].cpu().numpy(), want["rew"], "reward codes", case)
                _same(out["flags"].cpu().numpy(), want["flags"], "flags", case)
                _same(stats.cpu().numpy(), want["stats"], "stats", case)
                _state_same(vec.state(), want["state"], table, case)
                _same(vec.rule_audit()["bits"].cpu().numpy(), want["bits"][-1], "rule_audit() bits", case)
                _same(vec.audit_records(vec.snapshot())["bits"].cpu().numpy(), want["bits"][-1],
                      "audit_records() bits", case)


N_SAMPLE = 64


@functools.lru_cache(maxsize=None)
def _python_port(name):
    """oracle/rules_ref.py on 64 sampled final states of the oracle's rule trace (n = 300, traceback,
    next-step autoreset): env index, bits, {(x, y): region id}, fit mask.  Once per family."""
    proc = gp.rule_pool(name)[0]
    tr = gp.rule_trace(name, 300, T_RULES, True, "next_step")
    out = []
    for i in np.random.default_rng(17).choice(300, size=N_SAMPLE, replace=False):
        e = tr["saved"][int(i)]
        path = [list(pt) for pt in gp.env_path(e)]
        status = rules_ref.audit(dict(proc[e.pid]), path, (e.x, e.y))
        _, rm = rules_ref.RuleAudit(dict(proc[e.pid]), path, (e.x, e.y)).compute_regions()
        region = {(x, y): int(rm[x, y]) for x in range(rm.shape[0]) for y in range(rm.shape[1]) if rm[x, y] >= 0}
        fit = 0
        for d in status["poly_ylop_area"]["detail"].get("region_details", []):
            if d["ok"]:
                fit |= 1 << int(d["region"])
        out.append((int(i), rules_ref.rule_bits(status), region, fit))
    return out


@pytest.mark.parametrize("fit_cap", [None, 1])
@pytest.mark.parametrize("name", ALL)
def test_rule_audit_and_record_audit_vs_python_port(on_gpu, name, fit_cap):
    """rule_audit() (k_rules) and audit_records() (on one-word tab_all pools the table-only kernel)
    on the oracle's final states: bits of every env against the C oracle, the two audits against
    each other (bits, region map, fit mask), and bits, region map and fit mask of 64 sampled envs
    against the Python port.  fit_cap 1 sends nearly every exact-fit search to the host."""
    n = 300
    table = gp.rule_pool(name)[1]
    port = _python_port(gp.canonical(name))
    want = gp.rule_trace(name, n, T_RULES, True, "next_step")
    vec = _vec(name, n, True, rule=True, fit_cap=fit_cap)
    vec.reset(options={"puzzle_index": _pids(name, n, rule=True)})
    vec.rollout(T_RULES, _dev(gp.actions(name, n, T_RULES, rule=True)), record=False)
    case = (name, fit_cap)
    _state_same(vec.state(), want["state"], table, case)
    a = {k: v.cpu().numpy() for k, v in vec.rule_audit(region=True, fit=True).items()}
    b = {k: v.cpu().numpy() for k, v in vec.audit_records(vec.snapshot(), region=True, fit=True).items()}
    _same(a["bits"], want["bits"][-1], "rule_audit() bits", case)
    for k in ("bits", "region", "fit"):
        _same(b[k], a[k], f"audit_records() {k} vs rule_audit()", case)
    assert not (a["bits"] & (1 << 9)).any()
    for i, bits, region, fit in port:
        assert int(a["bits"][i]) == bits, (case, i)
        assert int(a["fit"][i].astype(np.uint64)) == fit, (case, i)
        row = np.full(64 * table.words, 255, np.uint8)
        for (x, y), r in region.items():
            row[x * table.pitch + y] = r
        _same(a["region"][i], row, "region map", (case, i))


# ----------------------------------------------------------------------------- (f) records
def _at_snap(name, n, tb, autoreset, rule=False):
    """A context after the first 20 steps of (a)'s run (of (e)'s for the rule pool), checked
    against the oracle's codes and flags, and the oracle's trace."""
    tr = (gp.rule_trace(name, n, T_RULES, tb, autoreset) if rule else gp.step_trace(name, n, T, tb, autoreset))
    v = _vec(name, n, tb, autoreset, rule=rule)
    v.reset(options={"puzzle_index": _pids(name, n, rule)})
    acts = gp.actions(name, n, T_RULES if rule else T, rule=rule)
    out = v.rollout(SNAP, _dev(acts[:SNAP]))
    _same(out["reward_code"].cpu().numpy(), tr["rew"][:SNAP], "reward codes", (name, tb, autoreset))
    _same(out["flags"].cpu().numpy(), tr["flags"][:SNAP], "flags", (name, tb, autoreset))
    return v, tr, acts


def _records_same(snap, saved, idx, proc, what):
    """Records against the oracle's env structs saved[idx[j]]: scalar fields, and with traceback
    the decoded path (tests/record_path.py asserts the record's own consistency)."""
    f = {k: np.asarray(v.cpu() if hasattr(v, "cpu") else v) for k, v in snap.fields().items()}
    envs = [saved[int(i)] for i in idx]
    for k, ko in (("x", "x"), ("y", "y"), ("path_len", "path_len"), ("step", "step"), ("puzzle_index", "pid")):
        _same(f[k], np.array([getattr(e, ko) for e in envs], np.int64), f"record field {k}", what)
    if snap.info.traceback:
        for j, (d, e) in enumerate(zip(record_path.decode(snap, snap.info, proc), envs)):
            assert d["path"] == gp.env_path(e), (what, j)


@pytest.mark.parametrize("tb", [True, False])
@pytest.mark.parametrize("name", ALL)
def test_records_decode_restore_fork(on_gpu, name, tb):
    """Snapshots at step 20, both autoreset modes: every record decodes to the oracle's path;
    restore followed by snapshot is the identity; fork with a rotation equals the oracle's copied
    structs, through the rest of the run."""
    n = 300
    proc, table, opool = gp.step_pool(name)
    src = (np.arange(n) + 65) % n
    for mode in MODES:
        case = (name, tb, mode)
        v, tr, acts = _at_snap(name, n, tb, mode)
        st = tr["state20"]
        assert (st["path_len"] > 3).any()
        if mode == "none":
            assert (st["pending"] != 0).any()                  # ended episodes stand among the records
        else:
            assert (st["pid"] != _pids(name, n)).any()         # and envs past an autoreset
        snap = v.snapshot()
        assert len(snap) == n and snap.info.words == table.words and snap.info.pitch == table.pitch
        _records_same(snap, tr["saved20"], np.arange(n), proc, case)
        w = _vec(name, n, tb, mode)                            # never reset: the restore covers every env
        _, info = w.restore(snap)
        _same(info["legal_mask"].cpu().numpy(), tr["legal20"], "legal masks after restore", case)
        assert torch.equal(w.snapshot().records, snap.records), case
        _, info = v.fork(src)
        _same(info["legal_mask"].cpu().numpy(), tr["legal20"][src], "legal masks after fork", case)
        assert torch.equal(v.snapshot().records, snap.records[_dev(src)]), case
        o = gp.oracle_from(opool, tr["saved20"], n, tb, gp.MAX_STEPS, mode, src)
        ro, fo = o.rollout(T - SNAP, acts[SNAP:])
        out = v.rollout(T - SNAP, _dev(acts[SNAP:]))
        _same(out["reward_code"].cpu().numpy(), ro, "reward codes after fork", case)
        _same(out["flags"].cpu().numpy(), fo, "flags after fork", case)
        _state_same(v.state(), o.state(), table, case)


@pytest.mark.parametrize("tb", [True, False])
@pytest.mark.parametrize("name", ALL)
def test_expand_children_and_oracle(on_gpu, name, tb):
    """expand() of the step-20 records: the children equal restore + one step + snapshot on a
    context of 4 n envs; codes, flags and legal masks equal the oracle's, stepped from the copied
    structs; both autoreset modes."""
    n = 300
    proc, table, opool = gp.step_pool(name)
    src4 = np.arange(4 * n) // 4
    a4 = (np.arange(4 * n) % 4).astype(np.uint8)
    for mode in MODES:
        case = (name, tb, mode)
        v, tr, _ = _at_snap(name, n, tb, mode)
        snap = v.snapshot()
        out = v.expand(snap)
        c = _vec(name, 4 * n, tb, mode)
        _, info = c.restore(snap, src=src4)
        rew = torch.empty(4 * n, dtype=torch.int8, device="cuda")
        flags = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
        c.core.step_device(_dev(a4).data_ptr(), rew.data_ptr(), flags.data_ptr())
        assert torch.equal(out["children"].records, c.snapshot().records), case
        o = gp.oracle_from(opool, tr["saved20"], 4 * n, tb, gp.MAX_STEPS, mode, src4)
        ro, fo = o.rollout(1, a4[None])
        for got in (out["reward_code"].cpu().numpy().reshape(-1), rew.cpu().numpy()):
            _same(got, ro[0], "reward codes", case)
        for got in (out["flags"].cpu().numpy().reshape(-1), flags.cpu().numpy()):
            _same(got, fo[0], "flags", case)
        _same(out["legal_mask"].cpu().numpy(), tr["legal20"], "legal masks", case)
        _records_same(out["children"], gp.save_envs(o), np.arange(4 * n), proc, case)
        v.core.sync()


@pytest.mark.parametrize("tb", [True, False])
@pytest.mark.parametrize("name", ALL)
def test_playout_traces_replayed_by_the_oracle(on_gpu, name, tb):
    """playout(K = 8, L = 32, trace) of the step-20 records: the traced actions, replayed by the
    oracle from the copied structs, are legal draws and give the returned codes, flags, steps,
    returns and final records; the first actions equal search.rand_pick."""
    from sparc_gym_amd.search import rand_pick
    n, K, L, seed = 300, 8, 32, 5
    proc, table, opool = gp.step_pool(name)
    v, tr, _ = _at_snap(name, n, tb, "none")                  # 'none': ended episodes stand among the records
    out = v.playout(v.snapshot(), K, L, seed=seed, trace=True, final=True)
    MK = n * K
    trace = out["trace"].cpu().numpy().reshape(L, MK)
    steps, code, flags, ret, first = (out[k].cpu().numpy().reshape(MK).astype(np.int64)
                                      for k in ("steps", "reward_code", "flags", "return", "first"))
    stepped_all = trace != 255
    assert np.array_equal(stepped_all.sum(0), steps) and (stepped_all[1:] <= stepped_all[:-1]).all()
    src = np.arange(MK) // K
    pending = tr["state20"]["pending"][src] != 0
    # 20 steps into episodes of at most 24, no playout reaches the horizon: each ends with its done step
    assert np.array_equal(steps == 0, pending) and pending.any() and (steps > 1).any()
    assert steps.max() <= gp.MAX_STEPS and ((flags & 1) != 0).any() and ((flags & 2) != 0).any()
    want_first = rand_pick(seed, np.arange(MK, dtype=np.uint64), 0, tr["legal20"][src].astype(np.int64))
    _same(first[~pending], np.asarray(want_first)[~pending], "first actions vs rand_pick", (name, tb))
    assert (first[pending] == 255).all() and np.array_equal(first[~pending], trace[0][~pending])
    o = gp.oracle_from(opool, tr["saved20"], MK, tb, gp.MAX_STEPS, "none", src)
    final = gp.save_envs(o)                                   # a playout without a step ends where it stood
    run = np.zeros(MK, np.int64)
    for t in range(L):
        legal = np.array([o.legal(i) for i in range(MK)], np.int64)
        stepped = stepped_all[t]
        assert (((legal >> np.minimum(trace[t], 3)) & 1) != 0)[stepped & (legal != 0)].all(), (name, tb, t)
        assert (trace[t][stepped & (legal == 0)] == 0).all()
        r, f = o.rollout(1, trace[t][None])                   # 255 is no action; an ended playout is not looked at again
        run += np.where(stepped, r[0], 0)
        last = stepped & (steps == t + 1)
        _same(r[0][last], code[last], "last reward codes", (name, tb, t))
        _same(f[0][last], flags[last], "last flags", (name, tb, t))
        _same(run[last], ret[last], "returns", (name, tb, t))
        assert (((f[0] & 3) != 0) | (t + 1 == L))[last].all() and ((f[0] & 3) == 0)[stepped & ~last].all()
        for i in np.flatnonzero(last):
            ctypes.memmove(ctypes.byref(final[i]), ctypes.byref(o.envs[i]), ctypes.sizeof(_Env))
    none = steps == 0
    assert (code[none] == 0).all() and (flags[none] == 0).all() and (ret[none] == 0).all()
    _records_same(out["final"], final, np.arange(MK), proc, (name, tb, "final records"))


DFS_ROOTS = 32


@pytest.mark.parametrize("budget", [7, 512])
@pytest.mark.parametrize("name", ALL)
def test_dfs_budget_and_resume_vs_walker(on_gpu, name, budget):
    """dfs(budget) from 32 live step-20 records of the rule pool's run (the leaves are audited, and
    the rule pool is the one whose exact-fit searches end in the reference too), continued twice:
    after each call the counters, the cursor's path and the first satisfying leaf equal
    dfs_ref.Walker.run(budget) below the oracle's path."""
    import dfs_ref
    n = 300
    proc = gp.rule_pool(name)[0]
    v, tr, _ = _at_snap(name, n, True, "next_step", rule=True)
    saved = tr["saved20"]
    live = [i for i in range(n) if not saved[i].pending][:DFS_ROOTS]
    assert len(live) == DFS_ROOTS and max(saved[i].path_len for i in live) > 3
    roots = v.snapshot(envs=np.asarray(live))
    _records_same(roots, saved, live, proc, (name, "roots"))
    inv = {d: a for a, d in dfs_ref.DIRS.items()}
    walkers = []
    for i in live:
        e = saved[i]
        path = gp.env_path(e)
        prefix = [inv[(b[0] - a[0], b[1] - a[1])] for a, b in zip(path[:-1], path[1:])]
        walkers.append(dfs_ref.Walker(proc[e.pid], prefix, max_steps=gp.MAX_STEPS, root_step=e.step))
    out = None
    for call in range(3):
        out = v.dfs(roots, budget) if out is None else v.dfs(out["cursor"], budget, state=out["state"],
                                                                counts=out["counts"], first=out["first"])
        counts, status = out["counts"].cpu().numpy(), out["status"].cpu().numpy()
        cursor, firsts, found = out["cursor"].moves(), out["first"].moves(), out["found"].cpu().numpy()
        for j, w in enumerate(walkers):
            w.run(budget)
            case = (name, budget, call, j)
            assert counts[j].tolist() == [w.counts[k] for k in dfs_ref.COUNTERS], case
            assert status[j] == (1 if w.complete else 2), case
            assert cursor[j] == w.path, case                   # the root's own path again when complete
            assert bool(found[j]) == (w.first is not None) and firsts[j] == (w.first or []), case
    assert (out["counts"][:, 7] == 0).all()                  # no leaf left undecided
    assert sum(w.counts["nodes"] for w in walkers) > DFS_ROOTS
    v.core.sync()
