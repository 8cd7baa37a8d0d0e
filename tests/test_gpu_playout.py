"""Legal-move playouts of state records on the GPU (SPaRCVecEnv.playout, sparc_playout_device).

Every output has an exact yardstick made from code that is already checked against the oracle:
the same playouts replayed ply by ply with ``expand`` (legal mask and children), the pop taken as
the child one point shorter than its parent, the draw by ``search.rand_pick`` and the chosen child
by ``select``; and, independently of ``expand``, the C oracle stepped with the traced actions.
Standing configuration of test_gpu_snapshot.py: 300 parents x 5 playouts = 1,500 lanes, five full
workgroups and a ragged one whose last wave has 28 lanes, records straddling wave boundaries;
max_steps 12 and horizon 6, so parents at step < 6 reach the horizon and later ones truncate."""
import numpy as np
import pytest

from sparc_gym_amd import _lib
from sparc_gym_amd.search import monte_carlo, rand_pick
from test_gpu_expand import MODES, _S, _ctx
from test_gpu_snapshot import N, STANDING, _arrays, _oracle, _same, _tables, _vec, _warm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K, L, SEED = 5, 6, 1
PER_PLAYOUT = ("reward_code", "flags", "steps", "first", "end", "return")


def _pending(rec):
    """aux bit 18 of host records [M, record_bytes]: the last step ended the episode"""
    return (rec[:, 6] >> 2) & 1 != 0


def _yardstick(v, snap, K, L, seed=0, id0=0, forward=False):
    """The playouts of `snap` replayed ply by ply on v.expand: numpy arrays under the names of
    SPaRCVecEnv.playout's result (per-playout arrays [M, K], trace [L, M, K], final [M * K,
    record_bytes], stats [M, 4, 4])."""
    from sparc_gym_amd.snapshot import Snapshot
    M = len(snap)
    MK = M * K
    g = np.arange(MK)
    ids = np.uint64(int(id0) & (2**64 - 1)) + g.astype(np.uint64)   # id0 is a 64-bit counter: it may pass 2^63
    cur = snap.select(g // K).numpy()
    live = ~_pending(cur)
    end = np.where(live, _lib.END_HORIZON, _lib.END_PENDING)
    code, flags, steps, ret = (np.zeros(MK, np.int64) for _ in range(4))
    first = np.full(MK, 255, np.int64)
    trace = np.full((L, MK), 255, np.uint8)
    for t in range(L):
        if not live.any():
            break
        parents = Snapshot(torch.from_numpy(cur).cuda(), snap.info)
        out = v.expand(parents)
        legal = out["legal_mask"].cpu().numpy().astype(np.int64)
        shorter = (out["children"].fields()["path_len"].reshape(MK, 4) < parents.fields()["path_len"][:, None])
        pop = (shorter.cpu().numpy() * (1 << np.arange(4))).sum(1) & legal
        # at most one pop (an ended parent under next-step autoreset has four reset children: not looked at)
        assert (np.bincount(pop[live], minlength=16)[[3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15]] == 0).all()
        mask = legal & ~pop if forward else legal
        dead = live & (mask == 0) & (legal != 0)
        end[dead] = _lib.END_DEAD_END
        live = live & ~dead
        a = rand_pick(seed, ids, t, mask)
        c = out["reward_code"].cpu().numpy()[g, a].astype(np.int64)
        f = out["flags"].cpu().numpy()[g, a].astype(np.int64)
        child = out["children"].records.cpu().numpy()[4 * g + a]
        first = np.where(live & (steps == 0), a, first)
        trace[t, live] = a[live]
        code, flags = np.where(live, c, code), np.where(live, f, flags)
        ret, steps = ret + np.where(live, c, 0), steps + live
        cur = np.where(live[:, None], child, cur)
        term, trunc = live & (f & 1 != 0), live & (f & 2 != 0)
        end[term], end[trunc] = _lib.END_TERMINATED, _lib.END_TRUNCATED
        live = live & ~(term | trunc)
    stats = np.zeros((M, 4, 4), np.int64)
    took = steps > 0
    for col, val in enumerate((took, took & (code == 100), took & (code == -100), steps)):
        np.add.at(stats[:, :, col], (g[took] // K, first[took]), val[took].astype(np.int64))
    sh = lambda x: x.reshape(M, K)  # noqa: E731
    return {"reward_code": sh(code), "flags": sh(flags), "steps": sh(steps), "first": sh(first), "end": sh(end),
            "return": sh(ret), "trace": trace.reshape(L, M, K), "final": cur, "stats": stats}


def _host(out):
    """a playout result on the host, the final snapshot as its records"""
    return {k: (x.records if k == "final" else x).cpu().numpy() for k, x in out.items()}


def _check_against(out, ref, M, K, L):
    assert set(out) == set(ref)
    for k in PER_PLAYOUT:
        assert out[k].shape == (M, K) and out[k].is_cuda, k
    assert out["reward_code"].dtype == torch.int8 and out["return"].dtype == torch.int32
    assert out["trace"].shape == (L, M, K) and out["trace"].dtype == torch.uint8
    assert len(out["final"]) == M * K and out["final"].records.is_cuda
    assert out["stats"].shape == (M, 4, 4) and out["stats"].dtype == torch.int32
    got = _host(out)
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k


def _play(v, snap, forward=False, **kw):
    args = dict(seed=SEED, forward_only=forward, trace=True, final=True)
    args.update(kw)
    return v.playout(snap, K, L, **args)


# ----------------------------------------------------------------------------- 1. chained expand
@pytest.mark.parametrize("forward", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,tb", STANDING)
def test_playouts_equal_chained_expand(on_gpu, name, tb, mode, forward):
    S = _S(name, tb)
    v = _ctx(S, mode)
    snap = v.snapshot()
    ref = _yardstick(v, snap, K, L, SEED, 0, forward)
    # on the yardstick's own results: every end reason this configuration can show is present
    reasons = set(np.unique(ref["end"]).tolist())
    want = {_lib.END_TERMINATED, _lib.END_TRUNCATED, _lib.END_HORIZON, _lib.END_PENDING}
    if forward and tb:
        want.add(_lib.END_DEAD_END)
    assert reasons == want
    assert (ref["steps"] == L).any() and (ref["steps"] == 0).any()
    _check_against(_play(v, snap, forward), ref, N, K, L)
    v.core.sync()


# ----------------------------------------------------------------------------- 2. the C oracle
@pytest.mark.parametrize("forward", [False, True])
@pytest.mark.parametrize("name,tb", STANDING)
def test_traced_actions_replayed_by_the_oracle(on_gpu, name, tb, forward):
    S = _S(name, tb)
    v = _warm(S)
    out = _host(_play(v, v.snapshot(), forward))
    MK = N * K
    trace = out["trace"].reshape(L, MK)
    steps, code, flags, ret = (out[k].reshape(MK).astype(np.int64) for k in ("steps", "reward_code", "flags", "return"))
    assert np.array_equal((trace != 255).sum(0), steps) and ((trace != 255)[1:] <= (trace != 255)[:-1]).all()
    o = _oracle(S, src=np.arange(MK) // K, autoreset="none", n=MK)
    run = np.zeros(MK, np.int64)
    for t in range(L):
        legal = np.array([o.legal(i) for i in range(MK)], np.int64)
        stepped = trace[t] != 255
        drawn = (legal >> np.minimum(trace[t], 3)) & 1 != 0
        assert drawn[stepped & (legal != 0)].all()
        assert (trace[t][stepped & (legal == 0)] == 0).all()
        r, f = o.rollout(1, trace[t][None])        # 255 is no action: an ended playout's env is not looked at again
        run += np.where(stepped, r[0], 0)
        last = stepped & (steps == t + 1)
        assert np.array_equal(r[0][last], code[last]) and np.array_equal(f[0][last], flags[last])
        assert np.array_equal(run[last], ret[last])
    none = steps == 0
    assert (code[none] == 0).all() and (flags[none] == 0).all() and (ret[none] == 0).all()


# ----------------------------------------------------------------------------- 3. no env involved
@pytest.mark.parametrize("name,tb", [("7x7_full", True), ("15x15", False)])
def test_env_state_untouched_and_no_reset_needed(on_gpu, name, tb):
    S = _S(name, tb)
    v = _warm(S)
    snap = v.snapshot()
    before = _arrays(v)
    warmed = _host(_play(v, snap, tb))
    v.core.sync()
    _same(_arrays(v), before)
    fresh = _host(_play(_vec(S), snap, tb))           # sparc_load_puzzles only
    for k in warmed:
        assert np.array_equal(fresh[k], warmed[k]), k
    host = v.core.playout_host(snap.info, snap.numpy(), K, L, seed=SEED, flags=int(tb), trace=True, final=True)
    for k, h in (("reward_code", "code"), ("return", "ret"), ("flags", "flags"), ("steps", "steps"),
                 ("first", "first"), ("end", "end"), ("trace", "trace"), ("final", "final"), ("stats", "stats")):
        assert np.array_equal(host[h], warmed[k]), k


# ----------------------------------------------------------------------------- 4. determinism, ids
@pytest.mark.parametrize("name,tb", [("7x7_full", True), ("mixed_5_11", False), ("15x15", True)])
def test_determinism_id_stream_and_stats(on_gpu, name, tb):
    S = _S(name, tb)
    v = _warm(S)
    snap = v.snapshot()
    full = _host(_play(v, snap, tb))
    again = _host(_play(v, snap, tb))
    for k in full:
        assert np.array_equal(again[k], full[k]), k
    a, b = 37, 250                                     # rows [a:b]: 1,065 playouts starting inside a wave
    part = _host(_play(v, snap.select(np.arange(a, b)), tb, id0=a * K))
    for k in PER_PLAYOUT + ("stats",):
        assert np.array_equal(part[k], full[k][a:b]), k
    assert np.array_equal(part["trace"], full["trace"][:, a:b])
    assert np.array_equal(part["final"], full["final"].reshape(N, K, -1)[a:b].reshape((b - a) * K, -1))
    other = _host(_play(v, snap, tb, id0=1))
    assert not np.array_equal(other["trace"], full["trace"])
    # stats: accumulated into the caller's array, and the host reduction of first / code / steps
    stats = torch.zeros((N, 4, 4), dtype=torch.int32, device="cuda")
    for _ in range(2):
        v.core.playout_device(snap.info, snap.records.data_ptr(), N, K, L, seed=SEED, flags=int(tb),
                              d_stats=stats.data_ptr())
    assert np.array_equal(stats.cpu().numpy(), 2 * full["stats"])
    want = np.zeros((N, 4, 4), np.int64)
    took = full["steps"] > 0
    j = np.broadcast_to(np.arange(N)[:, None], (N, K))
    for col, val in enumerate((took, took & (full["reward_code"] == 100), took & (full["reward_code"] == -100),
                               full["steps"])):
        np.add.at(want[:, :, col], (j[took], full["first"][took]), val[took].astype(np.int64))
    assert np.array_equal(full["stats"], want) and full["stats"][:, :, 0].sum() == took.sum()
    assert (full["first"][~took] == 255).all() and (full["first"][took] < 4).all()
    v.core.sync()


@pytest.mark.parametrize("K1", [1, 64, 200])
def test_stats_for_other_playouts_per_record(on_gpu, K1):
    """K = 1: 64 records per wave; 64: one record per wave; 200: a record over four waves."""
    S = _S("7x7_full", True)
    v = _warm(S)
    snap = v.snapshot().select(np.arange(9) * 31)
    out = v.playout(snap, K1, L, seed=SEED, forward_only=True, trace=True, final=True)
    _check_against(out, _yardstick(v, snap, K1, L, SEED, 0, True), 9, K1, L)
    v.core.sync()


# ----------------------------------------------------------------------------- 5. bad input
@pytest.mark.parametrize("name,tb", [("7x7_full", True), ("mixed_5_11", False)])
def test_damaged_records_are_refused_on_the_device(on_gpu, name, tb):
    from sparc_gym_amd.snapshot import Snapshot
    S = _S(name, tb)
    v = _warm(S)
    snap = v.snapshot()
    good = _host(_play(v, snap, tb))
    v.core.sync()
    rec = snap.records.clone()
    k_pid, k_len, k_x = 12, 130, 299          # 12: playouts 60-64 straddle a wave boundary; 299: the ragged wave
    P = len(S["proc"])
    rec[k_pid, 12:16] = torch.tensor(list(int(P).to_bytes(4, "little")), dtype=torch.uint8, device="cuda")
    rec[k_len, 2] = 0
    rec[k_x, 0] = max(int(p["x_size"]) for p in S["proc"])
    out = _host(_play(v, Snapshot(rec, snap.info), tb))
    with pytest.raises(ValueError, match="playout"):
        v.core.sync()
    v.core.sync()                                  # the error is reported once
    bad = np.zeros(N, bool)
    bad[[k_pid, k_len, k_x]] = True
    assert (out["end"][bad] == _lib.END_INVALID).all() and (out["first"][bad] == 255).all()
    assert (out["final"].reshape(N, K, -1)[bad] == 0).all() and (out["trace"][:, bad] == 255).all()
    for k in ("reward_code", "flags", "steps", "return", "stats"):
        assert (out[k][bad] == 0).all(), k
    for k in PER_PLAYOUT + ("stats",):
        assert np.array_equal(out[k][~bad], good[k][~bad]), k
    assert np.array_equal(out["trace"][:, ~bad], good["trace"][:, ~bad])
    assert np.array_equal(out["final"].reshape(N, K, -1)[~bad], good["final"].reshape(N, K, -1)[~bad])


def test_limits_and_flags_are_refused_on_the_host(on_gpu):
    S = _S("7x7_full", True)
    v = _warm(S)
    s = v.snapshot()
    end = torch.zeros(N * K, dtype=torch.uint8, device="cuda")
    call = lambda M=N, K=K, L=L, flags=0, rec=s.records.data_ptr(), **out: v.core.playout_device(  # noqa: E731
        s.info, rec, M, K, L, flags=flags, **(out or {"d_end": end.data_ptr()}))
    for kw, name in ((dict(M=0), "M must"), (dict(K=0), "K must"), (dict(M=2**16, K=2**15), r"M \* K"),
                     (dict(L=0), "L must"), (dict(L=65536), "L must"), (dict(M=1, K=2**16, L=2**15), r"K \* L"),
                     (dict(flags=2), "flags"), (dict(flags=1 | 1 << 31), "flags"), (dict(rec=None), "records"),
                     (dict(rec=s.records.data_ptr() + 8), "aligned"), (dict(d_final=end.data_ptr() + 8), "aligned"),
                     (dict(d_steps=end.data_ptr() + 1), "aligned"), (dict(d_stats=end.data_ptr() + 2), "aligned")):
        with pytest.raises(ValueError, match=name):
            call(**kw)
    with pytest.raises(ValueError, match="out"):
        v.core.playout_device(s.info, s.records.data_ptr(), N, K, L)
    for kw in (dict(playouts=0), dict(horizon=0), dict(horizon=65536), dict(playouts=2**23), dict(playouts=2**16,
                                                                                                 horizon=2**15)):
        with pytest.raises(ValueError):
            v.playout(s, **{"playouts": K, "horizon": L, **kw})
    with pytest.raises(ValueError, match="traceback"):
        _vec(S, traceback=False).playout(s, K, L)
    with pytest.raises(ValueError, match="traceback"):
        _vec(S, traceback=False).core.playout_device(s.info, s.records.data_ptr(), N, K, L, d_end=end.data_ptr())
    call()                                             # and the same call within the limits runs
    call(flags=1)
    v.core.sync()
    assert (end == 0).sum() == 0


def test_forward_flag_without_traceback_has_no_effect(on_gpu):
    S = _S("mixed_5_11", False)
    v = _warm(S)
    snap = v.snapshot()
    a, b = _host(_play(v, snap, False)), _host(_play(v, snap, True))
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ----------------------------------------------------------------------------- 6. a win is found
def test_a_win_is_found(on_gpu):
    """Forward-only walks from the reset state of four 7x7 puzzles, 256 each, to the end of the
    episode (a self-avoiding path has at most 49 points; horizon 64, max_steps 64)."""
    from sparc_gym_amd import SPaRCVecEnv
    K6, L6, seed = 256, 64, 3
    proc, table, _ = _tables("7x7_full")
    v = SPaRCVecEnv(4, processed=proc, table=table, traceback=True, max_steps=64, observation="compact")
    v.reset(options={"puzzle_index": np.arange(4)})
    snap = v.snapshot()
    ref = _yardstick(v, snap, K6, L6, seed, 0, True)
    won = (ref["reward_code"] == 100) & (ref["end"] == _lib.END_TERMINATED)
    assert won.any(1).all()                            # checked with the C oracle on the CPU beforehand
    assert set(np.unique(ref["end"]).tolist()) <= {_lib.END_TERMINATED, _lib.END_TRUNCATED, _lib.END_DEAD_END}
    out = v.playout(snap, K6, L6, seed=seed, forward_only=True, trace=True, final=True)
    _check_against(out, ref, 4, K6, L6)
    mc = monte_carlo(v, snap, K6, L6, seed=seed)
    assert np.array_equal(mc["visits"], ref["stats"][:, :, 0]) and np.array_equal(mc["wins"], ref["stats"][:, :, 1])
    assert mc["visits"].sum() == 4 * K6 and (mc["best_action"] >= 0).all()
    rows = torch.arange(4, device="cuda")
    for j, sol in enumerate(mc["solution"]):
        k = int(np.where(won[j], ref["steps"][j], 1 << 30).argmin())
        assert sol == ref["trace"][:ref["steps"][j, k], j, k].tolist() and len(sol) == ref["steps"][j].min(
            where=won[j], initial=1 << 30)
        cur = snap.select(rows[j:j + 1])               # replayed through expand: terminated with code +100
        for a in sol:
            e = v.expand(cur)
            assert (int(e["legal_mask"][0]) >> a) & 1
            code, flags = int(e["reward_code"][0, a]), int(e["flags"][0, a])
            cur = e["children"].select([a])
        assert code == 100 and flags & 3 == 1
    v.core.sync()
