"""Every rollout kernel family on small batches and short launches, bit for bit against the C oracle.

A case (tests/small_shapes.py) is one context stepped through small_shapes.launch_lengths back to
back: 0 to 5 full tiles with and without a short last tile, and past every ring and buffer count of
its kernel, at every env count of small_shapes.env_counts: below a wave, one wave, a partial
workgroup, whole workgroups and whole ones with a 1-env and a 16-env tail.  After every launch the
reward codes, flags, accumulated stats and, where the case produces them, the rule bits and both
observation planes equal the oracle's; after the last, so does the decoded state.  Every output
buffer is filled with a value no kernel writes before the launch, so a store that was skipped shows.

Which kernel a launch runs, what it sees of it, and what the oracle's trace must hold are asserted
without a GPU in tests/test_small_shapes_guards.py.  The second half runs the step and record entry
points on batches below and around one wave against the references their own files use."""
import numpy as np
import pytest

import small_shapes as ss
from oracle import COracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REW_FILL, FLAG_FILL, BITS_FILL, PLANE_FILL = 0x55, 0xAA, -21846, -7     # never a code, flags, bits or a cell
VARIANTS = {"IO_CODES_OFF": "VARIANT_IO_CODES_OFF", "RULE_ROLLOUT_GENERIC": "VARIANT_RULE_ROLLOUT_GENERIC",
            "R1R_SHAPE": "VARIANT_R1R_SHAPE", "OBS_INLINE": "VARIANT_OBS_INLINE"}


def _same(got, want, what, where):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, where, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        k = tuple(int(x) for x in bad[0])
        raise AssertionError(f"{what} differs at {len(bad)} of {want.size} places, first at (step, env, ...) or "
                             f"(env, ...) = {k}: got {got[k]}, oracle {want[k]}; {where}")


def test_pools_are_the_suites(on_gpu):
    from test_gpu_parity import POOLS
    for name, sizes in ss.STEP_SIZES.items():
        assert POOLS[name]["sizes"] == sizes and POOLS[name]["full_properties"]


@pytest.mark.parametrize("cid,n", ss.PARAMS, ids=[f"{cid}-n{n}" for cid, n in ss.PARAMS])
def test_rollout_small_shapes(on_gpu, cid, n):
    from sparc_gym_amd import SPaRCVecEnv
    from test_gpu_parity import _assert_states_equal
    c, P, tr = ss.CASE[cid], ss.pool(ss.CASE[cid]["pool"]), ss.trace(cid)
    pids = ss.puzzle_indices(c["pool"], n)
    vec = SPaRCVecEnv(n, processed=P.proc, table=P.table, traceback=c["tb"], autoreset=c["autoreset"],
                      observation="new" if c["obs"] else "compact", rules=c["rules"], max_steps=c["max_steps"],
                      env_offset=0 if c["given"] else ss.ENV_OFFSET)
    for k, v in c["variant"].items():
        vec.core.set_variant(getattr(vec.core, VARIANTS[k]), v)
    vec.reset(options={"puzzle_index": pids})
    acts = torch.from_numpy(tr.acts[:, :n].copy()).cuda() if c["given"] else None
    stats = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    X, Y = vec.x_dim, vec.y_dim
    if c["obs"]:   # the planes of the oracle: this batch's own, launch by launch (too large to keep per case)
        assert (X, Y) == (P.table.x_max, P.table.y_max)
        o = COracle(P.opool, n, c["tb"], c["max_steps"], autoreset=1)
        o.reset(pids)
    for li, want in enumerate(tr.launches):
        T, t0 = want["T"], want["t0"]
        where = f"launch {li} (steps {t0}..{t0 + T - 1}), case {cid}, n = {n}"
        a = None if acts is None else acts[t0:t0 + T]
        rew = torch.full((T, n), REW_FILL, dtype=torch.int8, device="cuda")
        flags = torch.full((T, n), FLAG_FILL, dtype=torch.uint8, device="cuda")
        if n % 16 == 0:                                       # what small_shapes.families takes for `tiled`
            assert all(t.data_ptr() % 16 == 0 for t in (rew, flags) + (() if a is None else (a,)))
        out = {}
        if c["rules"]:
            bits = torch.full((T, n), BITS_FILL, dtype=torch.int16, device="cuda")
            assert bits.data_ptr() % 16 == 0
            vec._stream()
            vec.core.rollout_rules_device(T, None if a is None else a.data_ptr(), rew.data_ptr(), flags.data_ptr(),
                                          stats.data_ptr(), bits.data_ptr(), c["seed"], t0)
            vec.core.rules_finish(bits.data_ptr())
            out["bits"] = bits
        elif c["obs"]:
            vis = torch.full((T, n, X, Y), PLANE_FILL, dtype=torch.int32, device="cuda")
            agent = torch.full((T, n, X, Y), PLANE_FILL, dtype=torch.int32, device="cuda")
            vec.rollout(T, a, seed=c["seed"], t0=t0, stats=stats, out=(rew, flags), obs_out=(vis, agent))
        else:
            vec.rollout(T, a, seed=c["seed"], t0=t0, stats=stats, out=(rew, flags))
        _same(rew.cpu().numpy(), want["rew"][:, :n], "reward codes", where)
        _same(flags.cpu().numpy(), want["flags"][:, :n], "flags", where)
        _same(stats.cpu().numpy(), want["stats"][:n], "stats", where)
        if c["rules"]:
            _same(out["bits"].cpu().numpy(), want["bits"][:, :n], "rule bits", where)
        if c["obs"]:
            ro, fo, vo, ao = o.rollout_obs(T, X, Y, None if a is None else tr.acts[t0:t0 + T, :n], seed=c["seed"],
                                           env_offset=0 if c["given"] else ss.ENV_OFFSET, t0=t0)
            assert np.array_equal(ro, want["rew"][:, :n]) and np.array_equal(fo, want["flags"][:, :n])
            for got, plane, what in ((vis, vo, "visited planes"), (agent, ao, "agent planes")):
                if not torch.equal(got, torch.from_numpy(plane).cuda()):
                    _same(got.cpu().numpy(), plane, what, where)
    _assert_states_equal(vec.state(), {k: v[:n] for k, v in tr.state.items()}, P.table)
    vec.core.sync()


# ----------------------------------------------------------------------------- step and record entry points
# Batches and record counts below and around one wave, each call against the reference its own test
# file uses: the C oracle from the standing state of tests/test_gpu_snapshot.py (a 48-step warm-up with
# pending envs and envs past an autoreset), restore + step + snapshot for expand, chained expand for
# playout, tests/rules_model.py for the audits and tests/dfs_ref.py for dfs.
SMALL = (1, 2, 3, 63, 64, 65)
STEP_POOLS = [("7x7_full", True), ("mixed_5_11", False), ("15x15", True)]


def _oracle_planes(o, X, Y):
    st = o.state()
    n = len(st["x"])
    agent = np.zeros((n, X, Y), np.int32)
    agent[np.arange(n), st["x"], st["y"]] = 1
    return st["visited"][:, :X, :Y].astype(np.int32), agent


@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("name,tb", STEP_POOLS)
def test_step_entry_points_below_a_wave(on_gpu, name, tb, n):
    """step_host, step_device, step (sparc_step_gym_device with 1-, 4- and 8-byte actions), obs_pack,
    copy_state / read_state, random_actions_device with T = 3 and a masked reset_device of the last
    env alone, on the standing state and its continuation under explicit actions."""
    import ctypes

    from test_gpu_parity import _assert_states_equal
    from test_gpu_snapshot import CONT, _arrays, _oracle, _run, _standing, _warm
    S = _standing(name, tb, n)
    v = _warm(S, observation="new")
    o = _oracle(S)
    acts, (ro, fo) = S["acts"], S["cont"]
    X, Y = v.x_dim, v.y_dim
    where = f"{name}, traceback {tb}, n = {n}"

    def oracle_step(t):
        r, f = o.rollout(1, acts[t:t + 1])
        assert np.array_equal(r[0], ro[t]) and np.array_equal(f[0], fo[t])

    r, f = v.core.step_host(acts[0])
    oracle_step(0)
    _same(r, ro[0], "step_host reward codes", where)
    _same(f, fo[0], "step_host flags", where)
    rew = torch.full((n,), REW_FILL, dtype=torch.int8, device="cuda")
    flags = torch.full((n,), FLAG_FILL, dtype=torch.uint8, device="cuda")
    a1 = torch.from_numpy(acts[1]).cuda()
    v.core.step_device(a1.data_ptr(), rew.data_ptr(), flags.data_ptr())
    oracle_step(1)
    _same(rew.cpu().numpy(), ro[1], "step_device reward codes", where)
    _same(flags.cpu().numpy(), fo[1], "step_device flags", where)
    odd = np.arange(n) % 2 == 1
    for t, dt, bad in ((2, np.uint8, 255), (3, np.int32, -3), (4, np.int64, 1 << 40)):
        a = np.where((acts[t] == 4) & odd, bad, acts[t].astype(np.int64)).astype(dt)     # every "no such action"
        obs, reward, term, trunc, info = v.step(torch.from_numpy(a).cuda())
        oracle_step(t)
        w = f"step with {np.dtype(dt).itemsize}-byte actions, {where}"
        _same(info["reward_code"].cpu().numpy(), ro[t], "reward codes", w)
        _same(reward.cpu().numpy(), ro[t].astype(np.float64) / 100.0, "rewards", w)
        _same(term.cpu().numpy(), (fo[t] & 1) != 0, "terminated", w)
        _same(trunc.cpu().numpy(), (fo[t] & 2) != 0, "truncated", w)
        _same(info["legal_mask"].cpu().numpy(), (fo[t] >> 2) & 0xF, "legal masks", w)
        _same(info["autoreset"].cpu().numpy(), (fo[t] & 64) != 0, "autoreset", w)
        vo, ao = _oracle_planes(o, X, Y)
        st = o.state()
        _same(obs["visited"].cpu().numpy(), vo, "visited planes", w)
        _same(obs["agent_location"].cpu().numpy(), ao, "agent planes", w)
        _same(obs["agent_xy"].cpu().numpy(), np.stack([st["x"], st["y"]], 1), "agent (x, y)", w)
        _same(obs["puzzle_index"].cpu().numpy(), st["pid"], "puzzle indices", w)
    vis = torch.full((n, X, Y), PLANE_FILL, dtype=torch.int32, device="cuda")
    agent = torch.full((n, X, Y), PLANE_FILL, dtype=torch.int32, device="cuda")
    v.core.obs_pack_device(vis.data_ptr(), agent.data_ptr(), X, Y)
    vo, ao = _oracle_planes(o, X, Y)
    _same(vis.cpu().numpy(), vo, "obs_pack visited planes", where)
    _same(agent.cpu().numpy(), ao, "obs_pack agent planes", where)
    s, arr = v.state(), _arrays(v)                                     # read_state and copy_state
    _assert_states_equal(s, o.state(), v.table)
    _same(arr[0].view(np.uint64), s["visited"], "copy_state visited words", where)
    _same(arr[1] & 0xFF, s["x"], "copy_state x", where)
    _same((arr[1] >> 8) & 0xFF, s["y"], "copy_state y", where)
    _same(arr[4], s["puzzle"].astype(np.int32), "copy_state puzzle index", where)
    drawn = torch.full((3, n), 0x77, dtype=torch.uint8, device="cuda")
    v.random_actions(3, seed=9, t0=5, out=drawn)
    _same(drawn.cpu().numpy(), np.array([[o.rand_action(9, i, 5 + t) for i in range(n)] for t in range(3)], np.uint8),
          "random_actions_device", where)
    # a masked reset of the last env alone; then the continuation of every env
    q = (o.state()["pid"] + 5) % len(S["proc"])
    mask = np.zeros(n, np.uint8)
    mask[-1] = 1
    flags = torch.full((n,), FLAG_FILL, dtype=torch.uint8, device="cuda")
    d_q, d_mask = torch.from_numpy(q.astype(np.int32)).cuda(), torch.from_numpy(mask).cuda()
    v.core.reset_device(d_q.data_ptr(), d_mask.data_ptr(), flags.data_ptr())
    assert o.lib.oracle_reset(ctypes.byref(o.pool.c), ctypes.byref(o.envs[n - 1]), int(q[-1])) == 0
    flags = flags.cpu().numpy()
    assert (flags[:-1] == FLAG_FILL).all() and flags[-1] == o.legal(n - 1) << 2, where
    _assert_states_equal(v.state(), o.state(), v.table)
    r, f = _run(v, acts[5:])
    ro2, fo2 = o.rollout(CONT - 5, acts[5:])
    _same(r, ro2, "reward codes after the masked reset", where)
    _same(f, fo2, "flags after the masked reset", where)
    _assert_states_equal(v.state(), o.state(), v.table)
    v.core.sync()


OTHER = {1: 65, 2: 63, 3: 64, 63: 2, 64: 3, 65: 1}     # M records into n != M envs


@pytest.mark.parametrize("M", SMALL)
@pytest.mark.parametrize("name,tb", STEP_POOLS)
def test_snapshot_restore_fork_below_a_wave(on_gpu, name, tb, M):
    """snapshot with a permuted env list; restore of those M records into n != M envs with a src
    gather and a mask; fork: the state arrays, the legal masks and the continuation against the
    oracle started from copies of its structs."""
    import ctypes

    from oracle import _Env
    from test_gpu_snapshot import CONT, MAX_STEPS, _arrays, _oracle, _run, _standing, _warm
    S, n2 = _standing(name, tb, M), OTHER[M]
    S2 = _standing(name, tb, n2)
    v = _warm(S)
    before = _arrays(v)
    rng = np.random.default_rng(M)
    perm = rng.permutation(M)
    snap = v.snapshot(envs=perm)
    assert len(snap) == M
    _same(snap.records.cpu().numpy(), v.snapshot().records.cpu().numpy()[perm], "records of a permuted env list", (name, M))
    b = _warm(S2)
    base = _arrays(b)
    src = rng.integers(M, size=n2)
    mask = np.arange(n2) % 2 == 0
    mask[-1] = True
    _, info = b.restore(snap, src=src, mask=mask)
    after = _arrays(b)
    for k in after:
        _same(after[k][..., mask], before[k][..., perm[src]][..., mask], f"restored state field {k}", (name, M))
        _same(after[k][..., ~mask], base[k][..., ~mask], f"state field {k} outside the mask", (name, M))
    legal = info["legal_mask"].cpu().numpy()
    assert (legal[~mask] == 0).all() and np.array_equal(legal[mask], S["legal"][perm[src]][mask])
    assert np.array_equal(info["restored"].cpu().numpy(), mask)
    o = COracle(S2["pool"], n2, tb, MAX_STEPS, autoreset=1)
    for i in range(n2):
        e = S["saved"][int(perm[src[i]])] if mask[i] else S2["saved"][i]
        ctypes.memmove(ctypes.byref(o.envs[i]), ctypes.byref(e), ctypes.sizeof(_Env))
    ro, fo = o.rollout(CONT, S2["acts"])
    r, f = _run(b, S2["acts"])
    _same(r, ro, "reward codes after the restore", (name, M))
    _same(f, fo, "flags after the restore", (name, M))
    # fork: a rotation by one (n = 1: onto itself)
    fsrc = (np.arange(M) + 1) % M
    _, info = v.fork(fsrc)
    after = _arrays(v)
    for k in after:
        _same(after[k], before[k][..., fsrc], f"forked state field {k}", (name, M))
    assert np.array_equal(info["legal_mask"].cpu().numpy(), S["legal"][fsrc])
    ro, fo = _oracle(S, fsrc).rollout(CONT, S["acts"])
    r, f = _run(v, S["acts"])
    _same(r, ro, "reward codes after the fork", (name, M))
    _same(f, fo, "flags after the fork", (name, M))
    v.core.sync()
    b.core.sync()


@pytest.mark.parametrize("M", SMALL)
@pytest.mark.parametrize("mode", ["next_step", "none"])
@pytest.mark.parametrize("name,tb", STEP_POOLS)
def test_expand_below_a_wave(on_gpu, name, tb, mode, M):
    """expand of M records: children, codes, flags and legal masks against restore, one step, snapshot."""
    from test_gpu_expand import _check_against, _composed, _ctx
    from test_gpu_snapshot import _standing
    S = _standing(name, tb, M)
    v = _ctx(S, mode)
    snap = v.snapshot()
    _check_against(v.expand(snap), _composed(S, snap, mode))
    v.core.sync()


@pytest.mark.parametrize("M,K", [(1, 1), (1, 3), (3, 1), (21, 3), (63, 1), (65, 1)])
@pytest.mark.parametrize("name,tb", STEP_POOLS)
def test_playout_below_a_wave(on_gpu, name, tb, M, K):
    """M * K = 1, 3, 63 and 65 playouts, stats and final records asked for, against the playouts
    replayed ply by ply on expand (itself restore, step and snapshot: the test above)."""
    import test_gpu_playout as pl
    from test_gpu_snapshot import _standing, _warm
    S = _standing(name, tb, M)
    v = _warm(S)
    snap = v.snapshot()
    for forward in (False, True):
        ref = pl._yardstick(v, snap, K, pl.L, pl.SEED, 0, forward)
        out = v.playout(snap, K, pl.L, seed=pl.SEED, forward_only=forward, trace=True, final=True)
        pl._check_against(out, ref, M, K, pl.L)
    v.core.sync()


@pytest.mark.parametrize("M", SMALL)
@pytest.mark.parametrize("pool", ["A", "C"])
def test_audit_records_below_a_wave(on_gpu, pool, M):
    """audit_records of M records on the table-only kernel (pool A, bits alone) and the generic one
    (region map and fit mask asked for; pool C: two words) against tests/rules_model.py's audit of
    the same states, after 20 steps of the small-shapes actions."""
    import rules_model
    from sparc_gym_amd import SPaRCVecEnv
    from sparc_gym_amd.puzzles import pack_rules
    P = ss.pool(pool)
    c = ss.CASE["k_rollout1r-A-tb1-next_step-given" if pool == "A" else "k_rollout_rules-C-tb1-next_step-given"]
    vec = SPaRCVecEnv(M, processed=P.proc, table=P.table, traceback=True, observation="compact", rules=True,
                      max_steps=c["max_steps"])
    vec.reset(options={"puzzle_index": ss.puzzle_indices(pool, M)})
    vec.rollout(20, torch.from_numpy(ss.trace(c["id"]).acts[:20, :M].copy()).cuda(), record=False)
    snap, st = vec.snapshot(), vec.state()
    aud = SPaRCVecEnv(1, processed=P.proc, table=P.table, traceback=True, observation="compact", max_steps=c["max_steps"])
    only = aud.audit_records(snap)["bits"].cpu().numpy()                  # pool A: k_rules_rec<1, true>
    gen = {k: x.cpu().numpy() for k, x in aud.audit_records(snap, region=True, fit=True).items()}
    rt_ = pack_rules(P.proc, P.table)
    W, seen = P.table.words, set()
    for j in range(M):
        vis = sum(int(st["visited"][k, j]) << (64 * k) for k in range(W))
        bits, fit, rmap = rules_model.audit(rt_, P.table, int(st["puzzle"][j]), vis, int(st["x"][j]), int(st["y"][j]))
        assert int(only[j]) == bits and int(gen["bits"][j]) == bits, (pool, M, j, int(only[j]), int(gen["bits"][j]), bits)
        seen.add(bits)
        assert int(gen["fit"][j].astype(np.uint64)) == fit, (pool, M, j)
        row = np.full(64 * W, 255, np.uint8)
        for b, r in rmap.items():
            row[b] = r
        _same(gen["region"][j], row, "region map", (pool, M, j))
    assert M < 63 or len(seen) > 1                                        # on the model's bits: states that differ
    aud.core.sync()


@pytest.mark.parametrize("M", SMALL)
def test_dfs_below_a_wave(on_gpu, M):
    """dfs of M roots as two launches of budget 7: counters, status, the cursor's path and the first
    satisfying leaf after each against dfs_ref.Walker.run(7)."""
    import dfs_ref
    from test_gpu_dfs import MAX_STEPS, make_vec, reset_roots
    proc = dfs_ref.pool("A")
    vec = make_vec("A", n=M)
    roots = reset_roots(vec, M)
    walkers = [dfs_ref.Walker(proc[j % len(proc)], max_steps=MAX_STEPS["A"]) for j in range(M)]
    out = None
    for call in range(2):
        out = vec.dfs(roots, 7) if out is None else vec.dfs(out["cursor"], 7, state=out["state"], counts=out["counts"],
                                                            first=out["first"])
        counts, status = out["counts"].cpu().numpy(), out["status"].cpu().numpy()
        cursor, firsts, found = out["cursor"].moves(), out["first"].moves(), out["found"].cpu().numpy()
        for j, w in enumerate(walkers):
            w.run(7)
            case = (M, call, j)
            assert counts[j].tolist() == [w.counts[k] for k in dfs_ref.COUNTERS], case
            assert status[j] == (1 if w.complete else 2), case
            assert cursor[j] == w.path, case
            assert bool(found[j]) == (w.first is not None) and firsts[j] == (w.first or []), case
    assert any(not w.complete for w in walkers)                           # the budget cut a walk short
    vec.core.sync()
