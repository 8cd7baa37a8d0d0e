"""Observation planes of state records on the GPU (SPaRCVecEnv.observe, search.solution_dataset,
sparc_observe_records_device / _host).

Yardsticks: the C oracle's state and legal masks after step 20 of the geometry pools' standing trace
(tests/geometry_pools.py; the trace of T = 53 steps that tests/test_gpu_geometry.py uses, whose
coverage floors are set for that length; the state after step 20 does not depend on T); the path the
project already has, checked against the oracle elsewhere: ``restore`` of the records into a second
env of M envs, its ``reset``-style observation (k_obs_pack) and its restore flags, and ``step`` for
the children of ``expand``; and tests/observe_ref.py, the numpy decoder that tests/test_observe_ref.py
checks against the oracle.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

import geometry_pools as gp
import golden_io
import observe_ref
import small_shapes as ss
from sparc_gym_amd import _lib
from sparc_gym_amd.search import actions_from_points, solution_dataset
from sparc_gym_amd.vec_env import OBS_DTYPES
from test_gpu_geometry import MODES, _at_snap, _dev, _same
from test_gpu_geometry import _vec as _gvec
from test_gpu_snapshot import MAX_STEPS, N, _arrays
from test_gpu_snapshot import _same as _same_arrays
from test_gpu_snapshot import _vec, _warm
from test_gpu_expand import _S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARITY = ("7x7_p8", "w1p4", "w1p12", "w2p7", "w2p15", "7x15_w2p16", "7x7_w4p7", "w4p13")
DTYPES = {torch.int32: (torch.int32, 1), torch.uint8: (torch.uint8, 1), torch.float16: (torch.int16, 0x3C00),
          torch.bfloat16: (torch.int16, 0x3F80), torch.float32: (torch.int32, 0x3F800000)}
KEYS = ("visited", "agent_location", "puzzle_index", "agent_xy", "legal_actions")
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257)
N_PARITY = 320


def _host(obs):
    return {k: obs[k].cpu().numpy() for k in KEYS}


def _agent_planes(x, y, xd, yd):
    a = np.zeros((len(x), xd, yd), np.int32)
    a[np.arange(len(x)), x, y] = 1
    return a


def _padded(v, xd, yd):
    """`v` with planes of xd x yd, as tests/test_gpu_geometry.py pads an env's."""
    v.x_dim, v.y_dim = xd, yd
    if v.observation == "new":
        v._vis = torch.empty((v.num_envs, xd, yd), dtype=torch.int32, device="cuda")
        v._agent = torch.empty_like(v._vis)
    return v


# ----------------------------------------------------------------------------- 1. oracle parity, byte parity
@pytest.mark.parametrize("tb", [True, False])
@pytest.mark.parametrize("name", PARITY)
def test_records_at_step_20_equal_the_oracle_and_the_env_path(on_gpu, name, tb):
    """320 envs, 20 steps of geometry_pools.actions under max_steps 24, snapshot, observe: the planes,
    the agent, the puzzle and the legal actions equal the oracle's state20 / legal20, pending records
    included; restore into a second env of 320 envs gives the same bytes through k_obs_pack and the
    restore flags; the children of expand observe as the restored parents' step() does."""
    n = N_PARITY
    proc, table, _ = gp.step_pool(name)
    src4 = np.arange(4 * n) // 4
    a4 = (np.arange(4 * n) % 4).astype(np.uint8)
    for mode in MODES:
        case = (name, tb, mode)
        v, tr, _ = _at_snap(name, n, tb, mode)
        gp.assert_step_coverage(name, tr, tb, mode)
        st, legal20 = tr["state20"], tr["legal20"]
        assert (st["path_len"] > 3).any() and len(np.unique(legal20)) > 4
        if mode == "none":
            assert (st["pending"] != 0).any()                  # ended episodes stand among the records
        snap = v.snapshot()
        xd, yd = v.x_dim, v.y_dim
        assert (xd, yd) == (table.x_max, table.y_max)
        ob = v.observe(snap)
        got = _host(ob)
        assert got["visited"].dtype == np.int32 and got["legal_actions"].dtype == np.uint8
        _same(got["visited"], st["visited"][:, :xd, :yd].astype(np.int32), "visited planes", case)
        _same(got["agent_location"], _agent_planes(st["x"], st["y"], xd, yd), "agent planes", case)
        _same(got["agent_xy"], np.stack([st["x"], st["y"]], 1).astype(np.int32), "agent_xy", case)
        _same(got["puzzle_index"], st["pid"].astype(np.int32), "puzzle_index", case)
        _same(got["legal_actions"], legal20, "legal_actions", case)
        dv, da, dp, dl = observe_ref.decode(snap.numpy(), table.words, table.pitch, xd, yd)
        assert np.array_equal(dv, got["visited"]) and np.array_equal(da, got["agent_location"]), case
        # the existing path: restore into M envs, the obs-pack observation, the restore flags
        w = _gvec(name, n, tb, mode, observation="new")
        o2, info = w.restore(snap)
        for k in KEYS[:4]:
            assert o2[k].dtype == torch.int32 and torch.equal(o2[k], ob[k]), (case, k)
        assert torch.equal(info["legal_mask"], ob["legal_actions"]), case
        # expand's children against step() of the restored parents
        oc = v.observe(v.expand(snap)["children"])
        c = _gvec(name, 4 * n, tb, mode, observation="new")
        c.restore(snap, src=src4)
        so, _, _, _, sinfo = c.step(_dev(a4))
        for k in KEYS[:4]:
            assert torch.equal(oc[k], so[k]), (case, k)
        assert torch.equal(oc["legal_actions"], sinfo["legal_mask"]), case
        v.core.sync()


# ----------------------------------------------------------------------------- 2. element types
@pytest.mark.parametrize("name", ["7x7_p8", "7x15_w2p16", "w4p13"])      # LUT one word, LUT two words, streams
def test_every_element_type_holds_the_int32_planes_in_two_patterns(on_gpu, name):
    n = 300
    v, _, _ = _at_snap(name, n, True, "next_step")
    snap = v.snapshot()
    ref = v.observe(snap)
    assert set(DTYPES) == set(OBS_DTYPES)
    for dt, (as_int, one) in DTYPES.items():
        out = v.observe(snap, dtype=dt)
        for k in KEYS[:2]:
            assert out[k].dtype == dt and out[k].shape == ref[k].shape
            assert torch.equal(out[k].to(torch.int32), ref[k]), (name, dt, k)
            raw = out[k].view(as_int).to(torch.int64) & (2 ** (8 * out[k].element_size()) - 1)
            assert set(torch.unique(raw).tolist()) == {0, one}, (name, dt, k)
        for k in KEYS[2:]:
            assert torch.equal(out[k], ref[k]), (name, dt, k)
    v.core.sync()


# ----------------------------------------------------------------------------- 3. small shapes and edges
SHAPE_CASES = [("7x7_full", 7, 7), ("7x7_full", 8, 8), ("7x7_full", 16, 16), ("mixed_5_11", None, None)]
_SMALL = {}


def _small(pool_name, tb=True):
    """300 records of a small_shapes pool after 20 random steps under max_steps 12 (computed once),
    their context, and per plane size the reference of all of them: the numpy decoder's planes and the
    restore path's puzzle, agent and legal actions."""
    if pool_name not in _SMALL:
        from sparc_gym_amd import SPaRCVecEnv
        P = ss.pool(pool_name)
        v = SPaRCVecEnv(N, processed=P.proc, table=P.table, traceback=tb, max_steps=MAX_STEPS, observation="compact")
        v.reset(options={"puzzle_index": ss.puzzle_indices(pool_name, N)})
        v.rollout(20, None, seed=5)
        snap = v.snapshot()
        w = SPaRCVecEnv(N, processed=P.proc, table=P.table, traceback=tb, max_steps=MAX_STEPS, observation="compact")
        o2, info = w.restore(snap)
        f = snap.fields()
        assert (f["path_len"] > 2).any() and len(torch.unique(f["puzzle_index"])) > 8
        _SMALL[pool_name] = dict(v=v, snap=snap, table=P.table, proc=P.proc, rec=snap.numpy(),
                                 puzzle=o2["puzzle_index"].cpu().numpy(), xy=o2["agent_location"].cpu().numpy(),
                                 legal=info["legal_mask"].cpu().numpy(), planes={})
    return _SMALL[pool_name]


def _small_ref(S, xd, yd):
    if (xd, yd) not in S["planes"]:
        t = S["table"]
        S["planes"][(xd, yd)] = observe_ref.decode(S["rec"], t.words, t.pitch, xd, yd)[:2]
    return S["planes"][(xd, yd)]


def _dims(S, xd, yd):
    return (S["table"].x_max, S["table"].y_max) if xd is None else (xd, yd)


@pytest.mark.parametrize("M", SIZES)
def test_small_shapes(on_gpu, M):
    """Every M around the wave and workgroup sizes, on the 7 x 7 pool at 49 cells (no element type
    makes a plane a whole number of 16-B pieces), padded to 8 x 8 (every type does) and to 16 x 16
    (the limit), and on mixed_5_11 (puzzles smaller than the planes: the padding cells are 0), in every
    element type."""
    rows = np.arange(M) * 7 % N
    for pool_name, xd, yd in SHAPE_CASES:
        S = _small(pool_name)
        xd, yd = _dims(S, xd, yd)
        v = _padded(S["v"], xd, yd)
        rv, ra = (p[rows] for p in _small_ref(S, xd, yd))
        if pool_name == "mixed_5_11":
            small = np.array([p["x_size"] < xd or p["y_size"] < yd for p in S["proc"]])[S["puzzle"][rows]]
            assert small.any() or M < 3
            for j in np.nonzero(small)[0]:
                p = S["proc"][int(S["puzzle"][rows[j]])]
                assert not rv[j, p["x_size"]:].any() and not rv[j, :, p["y_size"]:].any()
        snap = S["snap"].select(rows)
        for dt in DTYPES:
            case = (pool_name, xd, yd, M, dt)
            out = v.observe(snap, dtype=dt)
            assert out["visited"].shape == (M, xd, yd) and out["visited"].is_contiguous(), case
            _same(out["visited"].to(torch.int32).cpu().numpy(), rv, "visited planes", case)
            _same(out["agent_location"].to(torch.int32).cpu().numpy(), ra, "agent planes", case)
            _same(out["puzzle_index"].cpu().numpy(), S["puzzle"][rows], "puzzle_index", case)
            _same(out["agent_xy"].cpu().numpy(), S["xy"][rows], "agent_xy", case)
            _same(out["legal_actions"].cpu().numpy(), S["legal"][rows], "legal_actions", case)
        v.core.sync()


def _filled(shape, dt):
    """A tensor of `shape` and `dt` whose every byte is 0x5A."""
    numel = int(np.prod(shape))
    nbytes = numel * torch.empty(0, dtype=dt).element_size()
    return torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda").view(dt).view(shape)


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


@pytest.mark.parametrize("M", [65, 257])
def test_strided_output_touches_its_two_channels_only(on_gpu, M):
    """C = 5, channels (3, 1), the tensor pre-filled with 0x5A and one guard row allocated past its
    end: the two channels hold the dense result, every other byte is still 0x5A.  A 16-B piece that
    crossed a plane's end would show in channel 2, 4 or the guard."""
    rows = np.arange(M) * 7 % N
    C, cv, ca = 5, 3, 1
    for pool_name, xd, yd in SHAPE_CASES:
        S = _small(pool_name)
        xd, yd = _dims(S, xd, yd)
        v = _padded(S["v"], xd, yd)
        snap = S["snap"].select(rows)
        for dt in DTYPES:
            case = (pool_name, xd, yd, M, dt)
            dense = v.observe(snap, dtype=dt)
            big = _filled((M + 1, C, xd, yd), dt)
            out = v.observe(snap, dtype=dt, out=big[:M], channels=(cv, ca))
            assert out["visited"].data_ptr() == big[:, cv].data_ptr() and out["agent_location"].shape == (M, xd, yd)
            assert torch.equal(_bytes(big[:M, cv]), _bytes(dense["visited"])), case
            assert torch.equal(_bytes(big[:M, ca]), _bytes(dense["agent_location"])), case
            for k in KEYS[2:]:
                assert torch.equal(out[k], dense[k]), (case, k)
            assert (_bytes(big[:M, [0, 2, 4]]) == 0x5A).all(), case
            assert (_bytes(big[M]) == 0x5A).all(), case
        v.core.sync()


@pytest.mark.parametrize("M", [65, 257])
def test_a_plane_base_one_element_off_alignment(on_gpu, M):
    """Dense planes that start one element past a 16-B boundary take element stores: the same
    result, and the element before and the elements after are not written."""
    rows = np.arange(M) * 7 % N
    for pool_name, xd, yd in SHAPE_CASES[:2]:
        S = _small(pool_name)
        v = _padded(S["v"], xd, yd)
        snap = S["snap"].select(rows)
        rec = snap.records.contiguous()
        for dt in DTYPES:
            dense = v.observe(snap, dtype=dt)
            flat = [_filled((M * xd * yd + 9,), dt) for _ in range(2)]
            assert all(f.data_ptr() % 16 == 0 for f in flat)
            v._stream()
            v.core.observe_records_device(snap.info, rec.data_ptr(), M, OBS_DTYPES[dt], xd, yd, 0,
                                          d_visited=flat[0][1:].data_ptr(), d_agent=flat[1][1:].data_ptr())
            for f, k in zip(flat, KEYS[:2]):
                assert torch.equal(_bytes(f[1:1 + M * xd * yd]), _bytes(dense[k])), (pool_name, M, dt, k)
                assert (_bytes(f[:1]) == 0x5A).all() and (_bytes(f[1 + M * xd * yd:]) == 0x5A).all(), (pool_name, M, dt)
        v.core.sync()


# ----------------------------------------------------------------------------- 4. refusals on the device
@pytest.mark.parametrize("name,tb", [("7x7_full", True), ("mixed_5_11", False)])
def test_bad_records_are_refused_on_the_device(on_gpu, name, tb):
    """Zeroed, puzzle past the table, x or y outside, length 0, trie node past the count, mixed among
    good records (inside a wave, on both sides of a wave boundary, in the ragged wave): zero planes,
    puzzle_index -1, agent_xy (0, 0), legal_actions 0; the good ones exact; sync raises once."""
    from sparc_gym_amd.snapshot import Snapshot
    S = _S(name, tb)
    v = _warm(S)
    snap = v.snapshot()
    P = len(S["proc"])
    for dt, strided in ((torch.int32, False), (torch.uint8, False), (torch.float16, True)):
        def run(s):
            if not strided:
                return _host(v.observe(s, dtype=dt))
            big = _filled((N, 3, v.x_dim, v.y_dim), dt)
            o = _host(v.observe(s, dtype=dt, out=big, channels=(0, 2)))
            assert (_bytes(big[:, 1]) == 0x5A).all()
            return o

        good = run(snap)
        v.core.sync()
        rec = snap.records.clone()
        damage = {12: ("zero", None), 63: ("pid", P), 64: ("x", 200), 130: ("y", 200), 191: ("len", 0), 192: ("node", None),
                  299: ("pid", 2**32 - 1)}
        for k, (what, val) in damage.items():
            if what == "zero":
                rec[k] = 0
            elif what == "pid":
                rec[k, 12:16] = torch.tensor(list(int(val).to_bytes(4, "little")), dtype=torch.uint8, device="cuda")
            elif what == "node":
                rec[k, 4:6] = 0xFF
            else:
                rec[k, {"x": 0, "y": 1, "len": 2}[what]] = val
        out = run(Snapshot(rec, snap.info))
        with pytest.raises(ValueError, match="observe"):
            v.core.sync()
        v.core.sync()                                  # the error is reported once
        bad = np.zeros(N, bool)
        bad[list(damage)] = True
        as_int = np.uint8 if dt == torch.uint8 else (np.int32 if dt == torch.int32 else np.uint16)
        for k in KEYS[:2]:
            g, o = good[k].view(as_int), out[k].view(as_int)
            assert not o[bad].any() and np.array_equal(o[~bad], g[~bad]), (dt, k)
        assert (out["puzzle_index"][bad] == -1).all() and not out["agent_xy"][bad].any()
        assert not out["legal_actions"][bad].any()
        for k in KEYS[2:]:
            assert np.array_equal(out[k][~bad], good[k][~bad]), (dt, k)
        again = run(snap)                              # the next call is clean
        v.core.sync()
        for k in KEYS:
            assert np.array_equal(again[k].view(np.uint8), good[k].view(np.uint8)), (dt, k)


def test_arguments_are_refused_with_a_message(on_gpu):
    S = _S("7x7_full", True)
    v = _warm(S)
    s = v.snapshot()
    X, Y = v.x_dim, v.y_dim
    buf = torch.zeros(N * 256 * 4 + 64, dtype=torch.uint8, device="cuda")
    lib, ctx = v.core.lib, v.core.ctx

    def call(rec=s.records.data_ptr(), M=N, **kw):
        a = dict(visited=buf.data_ptr(), agent=None, elem=_lib.OBS_I32, x_dim=X, y_dim=Y, reserved=0, stride=0,
                 puzzle=None, loc=None, legal=None)
        a.update(kw)
        o = _lib.SparcObserveOut(**a)
        return lib.sparc_observe_records_device(ctx, ctypes.byref(s.info), rec, M, ctypes.byref(o))

    for kw, what in ((dict(elem=5), "elem"), (dict(elem=-1), "elem"), (dict(x_dim=X - 1), "x_dim"), (dict(y_dim=Y - 1), "y_dim"),
                     (dict(x_dim=16, y_dim=17), "x_dim"), (dict(x_dim=0), "x_dim"), (dict(stride=X * Y - 1), "stride"),
                     (dict(stride=-1), "stride"), (dict(M=0), "M must"), (dict(M=2**31), "M must"), (dict(rec=None), "records"),
                     (dict(rec=s.records.data_ptr() + 8), "aligned"), (dict(visited=buf.data_ptr() + 2), "aligned"),
                     (dict(agent=buf.data_ptr() + 1, elem=_lib.OBS_F16), "aligned"), (dict(visited=None), "at least one")):
        assert call(**kw) == -1, kw
        assert what in lib.sparc_last_error(ctx).decode(), (kw, lib.sparc_last_error(ctx))
    assert call() == 0 and call(stride=X * Y) == 0 and call(x_dim=16, y_dim=16) == 0
    assert call(visited=buf.data_ptr() + 3, elem=_lib.OBS_U8) == 0 and call(visited=None, legal=buf.data_ptr()) == 0
    v.core.sync()
    other = _vec(S, traceback=False)
    for bad_call in (lambda: other.observe(s), lambda: _vec(S, max_steps=MAX_STEPS + 1).observe(s)):
        with pytest.raises(ValueError, match="traceback|max_steps"):
            bad_call()
    with pytest.raises(ValueError, match="traceback"):
        other.core.observe_records_device(s.info, s.records.data_ptr(), N, d_visited=buf.data_ptr())


# ----------------------------------------------------------------------------- 5. no env, caller stream, host form
def test_no_env_is_touched_and_a_caller_stream_gives_the_same_bytes(on_gpu):
    from sparc_gym_amd.snapshot import Snapshot
    from test_gpu_streams import _Gate
    S = _S("mixed_5_11", True)
    v = _warm(S)
    snap = v.snapshot()
    table = S["table"]
    before, state = _arrays(v), v.state()
    ptrs = []
    for which in range(6):
        p = ctypes.c_void_p()
        assert v.core.lib.sparc_state_ptr(v.core.ctx, which, ctypes.byref(p)) == 0
        ptrs.append(p.value)
    own = _host(v.observe(snap, dtype=torch.float16))
    own32 = _host(v.observe(snap))
    v.core.sync()
    _same_arrays(_arrays(v), before)
    after = v.state()
    for k in state:
        assert np.array_equal(state[k], after[k]), k
    assert torch.equal(v.snapshot().records, snap.records)
    for which in range(6):
        p = ctypes.c_void_p()
        assert v.core.lib.sparc_state_ptr(v.core.ctx, which, ctypes.byref(p)) == 0 and p.value == ptrs[which]
    # a context that was never reset observes roots
    w = _vec(S)
    pz = np.arange(N) % len(S["proc"])
    roots = w.roots(pz)
    ro = _host(w.observe(roots))
    w.core.sync()
    assert w.core.has_state is False
    dv, da, dp, dl = observe_ref.decode(roots.numpy(), table.words, table.pitch, w.x_dim, w.y_dim)
    assert np.array_equal(ro["visited"], dv) and np.array_equal(ro["agent_location"], da)
    assert np.array_equal(ro["puzzle_index"], pz) and np.array_equal(ro["agent_xy"], dl)
    starts = np.array([S["proc"][q]["start_location"] for q in pz])
    assert np.array_equal(ro["agent_xy"], starts) and (ro["visited"].sum(axis=(1, 2)) == 1).all()
    # the host form, on an unaligned copy of the records
    raw = np.empty(snap.numpy().size + 1, np.uint8)
    un = raw[1:].reshape(snap.numpy().shape)
    un[:] = snap.numpy()
    assert un.ctypes.data % 2 == 1
    h = v.core.observe_records_host(snap.info, un)
    for k, hk in zip(KEYS, ("visited", "agent", "puzzle", "loc", "legal")):
        assert np.array_equal(h[hk].view(np.uint8), own32[k].view(np.uint8)), k
    h16 = v.core.observe_records_host(snap.info, un, elem=_lib.OBS_F16)
    assert np.array_equal(h16["visited"], own["visited"].view(np.uint16))
    assert np.array_equal(h16["agent"], own["agent_location"].view(np.uint16))
    # on a caller's stream: the true records arrive behind a gate on that stream; a launch on any
    # other stream reads the poison (the reset state's records)
    St = torch.cuda.Stream()
    true_r, buf_r = snap.records.clone(), v.roots(np.zeros(N, np.int64)).records.clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(St):
        gate = _Gate(St)
        buf_r.copy_(true_r, non_blocking=True)
        out = v.observe(Snapshot(buf_r, snap.info), dtype=torch.float16)
        gate.assert_closed("observe")
        assert v._bound_stream == St.cuda_stream
        St.synchronize()
        got = _host(out)
    for k in own:
        assert np.array_equal(got[k].view(np.uint8), own[k].view(np.uint8)), k


# ----------------------------------------------------------------------------- 6. solution_dataset
def test_solution_dataset_on_the_listed_solutions(on_gpu):
    from sparc_gym_amd import SPaRCVecEnv
    g = golden_io.load("rules_7x7_tb1")
    vec = SPaRCVecEnv(1, puzzles=g["records"], traceback=True, max_steps=2000, autoreset="none",
                      observation="compact")                 # one env: the batch plays no part
    ds = solution_dataset(vec)
    assert vec.core.has_state is False                        # loaded, never reset
    listed = [(q, k) for q, p in enumerate(g["processed"]) for k in range(len(p["solution_paths"]))]
    assert ds["skipped"] == {"wrong_start": 0, "non_unit_move": 0, "refused": 0} and ds["paths"] == listed
    sols = [g["processed"][q]["solution_paths"][k] for q, k in ds["paths"]]
    R = sum(len(s) - 1 for s in sols)
    assert R > 100 and all(ds[k].shape[0] == R for k in KEYS + ("action", "path", "t"))
    assert ds["visited"].dtype == torch.uint8 and ds["action"].dtype == torch.uint8
    h = {k: ds[k].cpu().numpy() for k in KEYS + ("action", "path", "t")}
    xd, yd = vec.x_dim, vec.y_dim
    r = 0
    for j, (sol, (q, _)) in enumerate(zip(sols, ds["paths"])):
        pts = [tuple(map(int, pt)) for pt in sol]
        acts, ok = actions_from_points(g["processed"][q]["start"], sol)
        assert ok
        for t in range(len(pts) - 1):
            vis, ag = np.zeros((xd, yd), np.uint8), np.zeros((xd, yd), np.uint8)
            for x, y in pts[:t + 1]:
                vis[x, y] = 1
            ag[pts[t]] = 1
            assert (h["path"][r], h["t"][r], h["puzzle_index"][r]) == (j, t, q), r
            assert np.array_equal(h["visited"][r], vis) and np.array_equal(h["agent_location"][r], ag), (j, t)
            assert tuple(h["agent_xy"][r]) == pts[t] and h["action"][r] == acts[t]
            dx, dy = ((1, 0), (0, -1), (-1, 0), (0, 1))[int(h["action"][r])]
            assert (pts[t][0] + dx, pts[t][1] + dy) == pts[t + 1]
            assert (h["legal_actions"][r] >> h["action"][r]) & 1, (j, t)
            r += 1
    assert r == R
    # a subset, another dtype, and listed paths that are left out
    sub = solution_dataset(vec, [3, 1], dtype=torch.float32)
    keep = [i for i, (q, _) in enumerate(ds["paths"]) if q in (1, 3)]
    assert sub["paths"] == [(q, k) for q in (3, 1) for k in range(len(g["processed"][q]["solution_paths"]))]
    assert sub["visited"].dtype == torch.float32 and sub["visited"].shape[0] == sum(len(sols[i]) - 1 for i in keep)
    import copy
    vec.puzzles = copy.deepcopy(vec.puzzles)
    p0 = vec.puzzles[0]
    assert len(p0["solution_paths"]) == 1
    first = [tuple(map(int, pt)) for pt in p0["solution_paths"][0]]
    assert first[0][0] == p0["x_size"] - 1                    # a move right from the start leaves the lattice
    p0["solution_paths"] = [first, first[1:], first[:2] + first[3:], first[:3] + first[:1],
                            [first[0], (first[0][0] + 1, first[0][1])]]
    cut = solution_dataset(vec, [0])
    assert cut["skipped"] == {"wrong_start": 1, "non_unit_move": 2, "refused": 1}
    assert cut["paths"] == [(0, 0)] and cut["action"].shape[0] == len(first) - 1
    assert torch.equal(cut["visited"], ds["visited"][:len(first) - 1])
    vec.core.sync()                                           # a path replay refuses is no device error
