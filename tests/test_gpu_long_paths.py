"""The step machine and the record kernels at long paths and at the lattice limits, against the
C oracle.

A kernel that keeps a path stores it as a 2-bit direction stack, 32 moves per 64-bit word, with
the length in 8 bits of `pos`.  These tests walk that encoding where it can go wrong: across the
word boundaries (moves 32, 64, 128, ...), back down across them by traceback pops, rewritten with
different moves after a walk back (so the multi-word stacks carry stale fields above the top), at
the largest length a lattice holds, and at 255 points, the largest length the field holds.

Pools (traceback on): gap-free 7x7 (one word, 49 points), 9x9 (two words), 15x15 (four words, 225
points) as test_gpu_splitw_edges.py makes them, and 16x16 with point (0, 0) closed and the start at
(0, 1): four words at pitch 16, 255 points.  16x16 is also the largest lattice the oracle judges.
On 16x16 both snakes repeat every 32 moves, the span of one stack word, so all stack words of a
scripted env hold the same fields there: a read of the wrong word shows on 15x15 (period 30) and
on the randomly stepping envs, whose paths pass 130 points on 16x16 within the script.

Every comparison is exact equality with the oracle; the decoded path of a record
(tests/record_path.py) is compared with the oracle's path[] point by point.  What a test relies on
(which kernel family a launch runs, the lengths reached, the pops across word boundaries) is
asserted on the dispatch conditions of sparc_rollout_device or on the oracle's state, never on the
output of the kernel under test."""
import ctypes
import functools

import numpy as np
import pytest

from long_pools import column_snake, row_snake, square_pool, walk
from oracle import COracle, OraclePool, _Env
from record_path import decode, encode
from small_shapes import base_families as _families   # the dispatch conditions of rollout_impl, restated once
from sparc_gym_amd import _lib
from sparc_gym_amd.puzzles import pack_table
from sparc_gym_amd.search import rand_pick
from test_gpu_parity import oracle_pool_from_processed
from test_gpu_snapshot import _copy_envs, _save_envs
from test_gpu_splitw_edges import _gap_free_pool, _snake

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MAX_STEPS = 100000
# name: lattice size, words, pitch, start, moves of the transposed snake walked after the walk back
SHAPES = {"7x7": (7, 1, 8, (0, 0), 40), "9x9": (9, 2, 9, (0, 0), 70), "15x15": (15, 4, 15, (0, 0), 140),
          "16x16": (16, 4, 16, (0, 1), 140)}
BOUNDARIES = (32, 64, 128)          # a stack word ends after this many moves

ENV_DT = np.dtype([(k, "<i4") for k in ("x", "y", "step", "outcome", "pid", "path_len", "pending", "pad")]
                  + [("path", "<i4", (257, 2)), ("visited", "u1", (16, 16))])
assert ENV_DT.itemsize == ctypes.sizeof(_Env)


def _view(envs):
    """the oracle's env structs as a numpy record array (no copy)"""
    return np.frombuffer(envs, ENV_DT)


@functools.lru_cache(maxsize=None)
def _pool(name):
    size, words, pitch, start, rewalk = SHAPES[name]
    proc = square_pool(16, closed=True) if name == "16x16" else _gap_free_pool((size - 1) // 2)
    table = pack_table(proc)
    assert (table.words, table.pitch) == (words, pitch)
    if name != "16x16":                                          # the table tests/test_tables_host.py checks
        twin = pack_table(square_pool(size, closed=False))
        assert np.array_equal(twin.open, table.open) and np.array_equal(twin.info, table.info)
    snake = column_snake(size, size, start[1])
    if start == (0, 0):
        assert snake == _snake(size, size)
    points = size * size - start[1]
    full = walk(start, snake)
    assert len(set(full)) == points == len(snake) + 1            # the snake covers every open point
    for p in proc:
        gaps = np.asarray(p["obs_array"]["gaps"])
        assert tuple(p["start_location"]) == start and int((gaps == 0).sum()) == points
        assert tuple(p["target_location"]) in ((size - 1, size - 1), (size - 1, 0))
    assert points <= 255 and (name != "16x16" or points == 255)
    again = row_snake(size, size)[:rewalk]
    assert len(set(walk(start, again))) == rewalk + 1 and max(b for _, b in walk(start, again)) < size
    assert sum(a != b for a, b in zip(snake, again)) > rewalk // 2    # the slots are rewritten with other moves
    return dict(name=name, proc=proc, table=table, opool=OraclePool(oracle_pool_from_processed(proc)), size=size,
                start=start, snake=snake, points=points, again=again)


def _vec(P, n, mode="none", max_steps=MAX_STEPS):
    from sparc_gym_amd import SPaRCVecEnv
    return SPaRCVecEnv(n, processed=P["proc"], table=P["table"], traceback=True, max_steps=max_steps, autoreset=mode,
                       observation="compact")


def _same_paths(records, info, P, ov):
    """every record's decoded path, board and scalars against the oracle's env structs `ov`"""
    dec = decode(records, info, P["proc"])
    assert len(dec) == len(ov)
    for i, (d, e) in enumerate(zip(dec, ov)):
        n = int(e["path_len"])
        assert (d["path_len"], d["x"], d["y"], d["puzzle"], d["step"]) == (n, e["x"], e["y"], e["pid"], e["step"]), i
        assert d["path"] == [tuple(pt) for pt in e["path"][:n].tolist()], f"record {i}: path"
        assert d["visited"] == set(zip(*(v.tolist() for v in np.nonzero(e["visited"])))), f"record {i}: board"


# ----------------------------------------------------------------------------- the action script
@functools.lru_cache(maxsize=None)
def _script(name, n, align):
    """"There and back": even envs walk the full snake, the reversed moves back to length 1, the
    first moves of the transposed snake, then 16 random actions; odd envs step randomly throughout.
    The script is cut into launches: at lengths 33, 65, 129 and points - 1 on the way out, at the
    full length, in the middle of the walk back, at length 1 and at the end.  With align = 16 every
    launch is padded to whole 16-step tiles with action 4 (no move).  Returns the actions [T, n],
    the launch boundaries, and {step: (cut name, the scripted envs' length there)}."""
    P = _pool(name)
    snake, S = P["snake"], len(P["snake"])
    back = [a ^ 2 for a in reversed(snake)]
    marks = sorted({b for b in BOUNDARIES if b < S} | {S - 1})
    pieces = [snake[a:b] for a, b in zip([0] + marks, marks + [S])] + [back[:S // 2], back[S // 2:], P["again"]]
    lengths = [b + 1 for b in marks] + [S + 1, S + 1 - S // 2, 1, len(P["again"]) + 1]
    names = [None] * len(marks) + ["full", "mid_back", "one", None]
    script, bounds, cuts = [], [0], {}
    for piece, length, cut in zip(pieces, lengths, names):
        script += piece + [4] * (-len(piece) % align)
        bounds.append(len(script))
        cuts[len(script)] = (cut, length)
    T = len(script) + 16
    bounds.append(T)
    cuts[T] = ("end", None)
    rng = np.random.default_rng(len(name) * 1000 + n)
    acts = rng.integers(0, 4, (T, n)).astype(np.uint8)
    acts[:len(script), 0::2] = np.asarray(script, np.uint8)[:, None]
    assert {33, 65, 129, P["points"] - 1} & set(range(P["points"])) <= {c[1] for c in cuts.values()}
    return acts, bounds, cuts


FAMILY = {"k_step": (64, 1), "k_rollout1s": (256, 16), "k_rollout1": (300, 1), "k_rolloutWs": (512, 16),
          "k_rollout": (300, 1)}
CASES = [(name, "k_step", "none") for name in SHAPES] + [
    ("7x7", "k_rollout1s", "none"), ("7x7", "k_rollout1", "none"), ("9x9", "k_rolloutWs", "none"),
    ("15x15", "k_rolloutWs", "none"), ("9x9", "k_rollout", "none"), ("15x15", "k_rollout", "none"),
    ("16x16", "k_rollout", "none"),
    # next-step autoreset: the reset after the full snake clears a long stack
    ("7x7", "k_step", "next_step"), ("7x7", "k_rollout1s", "next_step"), ("7x7", "k_rollout1", "next_step"),
    ("9x9", "k_rolloutWs", "next_step"), ("15x15", "k_rolloutWs", "next_step"), ("15x15", "k_rollout", "next_step"),
    ("16x16", "k_rollout", "next_step"), ("16x16", "k_step", "next_step")]


@pytest.mark.parametrize("name,family,mode", CASES)
def test_there_and_back(on_gpu, name, family, mode):
    """a. every kernel family runs the script; after every launch the reward codes, flags, stats
    and lengths equal the oracle's, and at the cut points so does every env's decoded path.
    k_step is driven action by action through sparc_step_device (one launch per step, no stats);
    the rollout families by one sparc_rollout_device call per piece of the script, each of which
    must run the one family by the dispatch conditions (_families)."""
    P = _pool(name)
    n, align = FAMILY[family]
    acts, bounds, cuts = _script(name, n, align)
    T = bounds[-1]
    max_steps = MAX_STEPS if mode == "none" else T + 3      # just above the script: no step-count truncation
    pids = np.arange(n) % len(P["proc"])
    v = _vec(P, n, mode, max_steps)
    v.reset(options={"puzzle_index": pids})
    o = COracle(P["opool"], n, True, max_steps, autoreset=int(mode == "next_step"))
    o.reset(pids)
    ov = _view(o.envs)
    info = v.core.snapshot_info()
    d_acts = torch.from_numpy(acts).cuda()
    stats = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    ost = np.zeros((n, 4), np.int32)
    reached, longest_random = set(), 0
    for a, b in zip(bounds[:-1], bounds[1:]):
        ro, fo = o.rollout(b - a, acts[a:b], stats=ost)
        if family == "k_step":
            rew = torch.empty((b - a, n), dtype=torch.int8, device="cuda")
            flags = torch.empty((b - a, n), dtype=torch.uint8, device="cuda")
            for t in range(b - a):
                v.core.step_device(d_acts[a + t].data_ptr(), rew[t].data_ptr(), flags[t].data_ptr())
        else:
            assert _families(P["table"], n, b - a) == {family}
            out = v.rollout(b - a, d_acts[a:b], stats=stats)
            rew, flags = out["reward_code"], out["flags"]
            if n % 16 == 0:                                       # the tiled kernels need 16-B aligned buffers
                assert d_acts[a:b].data_ptr() % 16 == 0 and rew.data_ptr() % 16 == 0 and flags.data_ptr() % 16 == 0
            assert np.array_equal(stats.cpu().numpy(), ost), f"stats after step {b}"
        assert np.array_equal(rew.cpu().numpy(), ro), f"reward codes of steps {a}..{b}"
        assert np.array_equal(flags.cpu().numpy(), fo), f"flags of steps {a}..{b}"
        assert np.array_equal(v.state()["path_len"].astype(np.int64), ov["path_len"]), f"lengths after step {b}"
        longest_random = max(longest_random, int(ov["path_len"][1::2].max()))
        cut, length = cuts[b]
        if mode == "none" and length is not None:               # the script does what it says, on the oracle
            assert (ov["path_len"][0::2] == length).all(), (cut, length)
            reached.add(length)
        if cut is not None:
            _same_paths(v.snapshot(), info, P, ov)
    v.core.sync()
    if mode == "none":
        assert {P["points"], P["points"] - 1, 1} <= reached
        assert {b + 1 for b in BOUNDARIES if b < P["points"] - 1} <= reached
        if name == "16x16":       # the envs whose stack words differ from each other use the fifth word too
            assert longest_random > 130
    else:
        # every scripted env was reset at a long length: its first episode ended at the target, in
        # the last column of the snake (the oracle's autoreset count)
        assert (ost[0::2, 3] >= 1).all()


# ----------------------------------------------------------------------------- records at every length
@functools.lru_cache(maxsize=None)
def _ladder(name):
    """The oracle's side of two envs (puzzles 0 and 1: both target corners) stepped through the
    snake, back to length 1 and through the transposed snake: the actions, and the oracle's structs
    and legal masks after every step (index 0: the reset state)."""
    P = _pool(name)
    snake = P["snake"]
    acts = snake + [a ^ 2 for a in reversed(snake)] + P["again"]
    o = COracle(P["opool"], 2, True, MAX_STEPS, autoreset=0)
    o.reset([0, 1])
    saved, legal = [_save_envs(o)], [[o.legal(0), o.legal(1)]]
    for a in acts:
        o.rollout(1, np.full((1, 2), a, np.uint8))
        saved.append(_save_envs(o))
        legal.append([o.legal(0), o.legal(1)])
    lens = np.array([[s[0].path_len, s[1].path_len] for s in saved])
    S = len(snake)
    assert (lens[:S + 1, 0] == np.arange(1, S + 2)).all() and (lens[2 * S] == 1).all()
    assert (lens[2 * S:, 1] == np.arange(1, len(P["again"]) + 2)).all()
    return dict(acts=acts, saved=saved, legal=np.asarray(legal, np.uint8), lens=lens, S=S)


def _ladder_snapshots(P, Ld, steps):
    """Records of the two envs after each step in `steps` (sorted), from a context stepped with
    k_step; checked against the oracle's paths.  Returns (Snapshot on the GPU, the oracle's structs
    in record order, the legal masks)."""
    from sparc_gym_amd.snapshot import Snapshot
    v = _vec(P, 2)
    v.reset(options={"puzzle_index": np.arange(2)})
    d_acts = torch.from_numpy(np.repeat(np.asarray(Ld["acts"], np.uint8)[:, None], 2, 1)).cuda()
    rew = torch.empty(2, dtype=torch.int8, device="cuda")
    flags = torch.empty(2, dtype=torch.uint8, device="cuda")
    want, snaps = set(steps), []
    for t in range(max(steps) + 1):
        if t > 0:
            v.core.step_device(d_acts[t - 1].data_ptr(), rew.data_ptr(), flags.data_ptr())
        if t in want:
            snaps.append(v.snapshot())
    v.core.sync()
    snap = Snapshot.cat(snaps)
    structs = (_Env * (2 * len(steps)))()
    for k, t in enumerate(sorted(steps)):
        ctypes.memmove(ctypes.byref(structs[2 * k]), Ld["saved"][t], 2 * ctypes.sizeof(_Env))
    _same_paths(snap, snap.info, P, _view(structs))
    return snap, structs, np.concatenate([Ld["legal"][t] for t in sorted(steps)])


@pytest.mark.parametrize("name", list(SHAPES))
def test_expand_at_every_length(on_gpu, name):
    """b. parents at every length 1 .. points on the way out, at every eighth length on the way
    back and at every length of the re-walk (multi-word parents then carry stale fields above the
    top): codes, flags and legal masks against the oracle stepped from copies of its envs, each
    child's decoded path against the oracle's, and the children byte for byte against restore,
    one step, snapshot."""
    P, Ld = _pool(name), _ladder(name)
    S = Ld["S"]
    steps = sorted(set(range(S + 1)) | set(range(S, 2 * S, 8)) | set(range(2 * S, len(Ld["acts"]) + 1)))
    snap, structs, legal = _ladder_snapshots(P, Ld, steps)
    M = len(snap)
    assert M == 2 * len(steps) <= 1000
    lens = _view(structs)["path_len"]
    assert set(range(1, P["points"] + 1)) <= set(lens[:2 * (S + 1)].tolist())
    v = _vec(P, 2)                                              # its tables only: never reset
    out = v.expand(snap)
    o4 = COracle(P["opool"], 4 * M, True, MAX_STEPS, autoreset=0)
    _copy_envs(o4, structs, np.arange(4 * M) // 4)
    a4 = (np.arange(4 * M) % 4).astype(np.uint8)
    ro, fo = o4.rollout(1, a4[None])
    assert np.array_equal(out["reward_code"].cpu().numpy().reshape(-1), ro[0])
    assert np.array_equal(out["flags"].cpu().numpy().reshape(-1), fo[0])
    assert np.array_equal(out["legal_mask"].cpu().numpy(), legal)
    _same_paths(out["children"], snap.info, P, _view(o4.envs))
    # pops are among the children at every length >= 2, and pushes across every boundary
    clen = _view(o4.envs)["path_len"].reshape(M, 4)
    assert ((clen < lens[:, None]).sum(1) == (lens >= 2)).all()
    for b in (b for b in BOUNDARIES if b + 2 <= P["points"]):
        assert (clen[lens == b + 1] == b + 2).any() and (clen[lens == b + 2] == b + 1).any()
    c = _vec(P, 4 * M)
    c.restore(snap, src=np.arange(4 * M) // 4)
    rew = torch.empty(4 * M, dtype=torch.int8, device="cuda")
    flags = torch.empty(4 * M, dtype=torch.uint8, device="cuda")
    c.core.step_device(torch.from_numpy(a4).cuda().data_ptr(), rew.data_ptr(), flags.data_ptr())
    assert np.array_equal(out["children"].records.cpu().numpy(), c.snapshot().records.cpu().numpy())
    assert np.array_equal(rew.cpu().numpy(), ro[0]) and np.array_equal(flags.cpu().numpy(), fo[0])
    v.core.sync()
    c.core.sync()


def test_one_word_parents_with_fields_above_the_top(on_gpu):
    """A one-word record is canonical (only the path's moves set); restore, expand and playout are
    documented to mask a record that is not.  Parents at lengths 32, 33 and 34 with every field above
    the top set give the children, playouts and restored state of the canonical parents."""
    from sparc_gym_amd.snapshot import Snapshot
    P, Ld = _pool("7x7"), _ladder("7x7")
    snap, structs, _ = _ladder_snapshots(P, Ld, [31, 32, 33])
    info = snap.info
    clean = snap.records.cpu().numpy()
    lens = _view(structs)["path_len"]
    assert lens.tolist() == [32, 32, 33, 33, 34, 34]
    dirty = clean.copy()
    for row, n in zip(dirty, lens):
        d = decode(row[None], info, P["proc"])[0]
        row[:] = encode(info, d["puzzle"], d["path"], stale={k: 1 + k % 3 for k in range(n - 1, 64)},
                        step=d["step"], aux=int(row[4:8].view("<u4")[0]), off=int(row[3]))
    assert not np.array_equal(dirty, clean) and np.array_equal(dirty[:, :24], clean[:, :24])
    v = _vec(P, 6)
    a, b = Snapshot(torch.from_numpy(clean).cuda(), info), Snapshot(torch.from_numpy(dirty).cuda(), info)
    ea, eb = v.expand(a), v.expand(b)
    assert torch.equal(ea["children"].records, eb["children"].records) and torch.equal(ea["flags"], eb["flags"])
    pa, pb = (v.playout(s, 8, 48, seed=1, trace=True, final=True) for s in (a, b))
    assert torch.equal(pa["trace"], pb["trace"]) and torch.equal(pa["final"].records, pb["final"].records)
    v.restore(b)
    assert np.array_equal(v.snapshot().records.cpu().numpy(), clean)
    v.core.sync()


# ----------------------------------------------------------------------------- playouts from deep records
PARENT_LENGTHS = (2, 32, 33, 34, 64, 65, 66, 97, 129, 193, 224, 225, 255)
K, L = 8, 48
# The first seed in 1, 2, 3, ... for which the oracle's own playouts (drawn with rand_pick from the
# oracle's legal sets, no GPU) pop across every word boundary the pool has and push across one
# again; chosen by the oracle, asserted by every run on the oracle's replay of the kernel's trace.
SEEDS = {"7x7": 1, "9x9": 1, "15x15": 1, "16x16": 1}


def _oracle_playouts(name, forward, seed, trace=None):
    """K playouts of at most L steps from the parents of PARENT_LENGTHS on the oracle: drawn with
    rand_pick from the oracle's legal sets (trace None), or replayed from `trace` [L, M * K], every
    action of which must then be in the oracle's legal set.  Returns what k_playout reports, the
    oracle's structs at each playout's end, and the lengths each playout went through."""
    P, Ld = _pool(name), _ladder(name)
    steps = [n - 1 for n in PARENT_LENGTHS if n <= P["points"]]
    M = 2 * len(steps)
    MK = M * K
    o = COracle(P["opool"], MK, True, MAX_STEPS, autoreset=0)
    for k, t in enumerate(steps):
        for j in range(2):
            for r in range(K):
                ctypes.memmove(ctypes.byref(o.envs[(2 * k + j) * K + r]), ctypes.byref(Ld["saved"][t][j]),
                               ctypes.sizeof(_Env))
    ov = _view(o.envs)
    g = np.arange(MK)
    live = ov["pending"] == 0
    end = np.where(live, _lib.END_HORIZON, _lib.END_PENDING)
    code, flags, nsteps, ret = (np.zeros(MK, np.int64) for _ in range(4))
    out_trace = np.full((L, MK), 255, np.uint8)
    final = (_Env * MK)()
    ctypes.memmove(final, o.envs, ctypes.sizeof(final))
    fv = _view(final)
    lens = [ov["path_len"].copy()]
    for t in range(L):
        legal = np.array([o.legal(i) for i in range(MK)], np.int64)
        n = ov["path_len"]
        prev = ov["path"][g, np.maximum(n - 2, 0)]                       # path[-2]
        d = prev - np.stack([ov["x"], ov["y"]], 1)
        pop = np.zeros(MK, np.int64)
        for a, (dx, dy) in enumerate(((1, 0), (0, -1), (-1, 0), (0, 1))):
            pop |= ((n >= 2) & (d[:, 0] == dx) & (d[:, 1] == dy)).astype(np.int64) << a
        assert ((pop & legal) == pop).all()                              # the way back is always legal
        mask = legal & ~pop if forward else legal
        dead = live & (mask == 0) & (legal != 0)                         # the oracle's legal set is exactly the pop
        end[dead] = _lib.END_DEAD_END
        live = live & ~dead
        if trace is None:
            a = rand_pick(seed, g, t, mask)
        else:
            a = trace[t].astype(np.int64)
            assert ((a != 255) == live).all(), f"step {t}: the kernel stepped other playouts than the oracle"
            a = np.where(live, a, 0)
            assert (((mask >> a) & 1) != 0)[live & (mask != 0)].all(), f"step {t}: an action outside the legal set"
            assert (a[live & (mask == 0)] == 0).all()
        out_trace[t, live] = a[live]
        r, f = o.rollout(1, np.where(live, a, 255).astype(np.uint8)[None])
        r, f = r[0].astype(np.int64), f[0].astype(np.int64)
        code, flags = np.where(live, r, code), np.where(live, f, flags)
        ret, nsteps = ret + np.where(live, r, 0), nsteps + live
        fv[live] = ov[live]
        lens.append(np.where(live, ov["path_len"], -1))
        term, trunc = live & (f & 1 != 0), live & (f & 2 != 0)
        end[term], end[trunc] = _lib.END_TERMINATED, _lib.END_TRUNCATED
        live = live & ~(term | trunc)
    first = np.where(nsteps > 0, out_trace[0], 255)
    return dict(M=M, steps=steps, reward_code=code, flags=flags, nsteps=nsteps, ret=ret, end=end, first=first,
                trace=out_trace, final=final, lens=np.stack(lens))


def _crossings(lens, points):
    """(boundaries b some playout popped across: its length was >= b + 2 and later <= b; whether one
    pushed back across: ... and later >= b + 2 again), on the oracle's lengths [L + 1, MK]."""
    popped, pushed = set(), False
    for b in (b for b in BOUNDARIES if b + 2 <= points):
        for col in lens.T:
            col = col[col >= 0]
            hi = np.flatnonzero(col >= b + 2)
            if not len(hi):
                continue
            lo = np.flatnonzero(col[hi[0]:] <= b)
            if len(lo):
                popped.add(b)
                pushed = pushed or bool((col[hi[0] + lo[0]:] >= b + 2).any())
    return popped, pushed


def _covered(name, sims):
    """the coverage the seed must give, over the playouts with and without the pop"""
    P = _pool(name)
    want = {b for b in BOUNDARIES if b + 2 <= P["points"]}
    popped, pushed = _crossings(sims[False]["lens"], P["points"])
    ends = set(sims[True]["end"].tolist()) | set(sims[False]["end"].tolist())
    # a parent at the full length has ended its episode where the snake's end is the target
    reasons = {_lib.END_HORIZON} | ({_lib.END_PENDING} if P["points"] in PARENT_LENGTHS else set())
    return popped == want and pushed and _lib.END_DEAD_END in set(sims[True]["end"].tolist()) and reasons <= ends


@pytest.mark.parametrize("name", list(SHAPES))
def test_playouts_from_deep_records(on_gpu, name):
    """c. K = 8 playouts of 48 steps from parents at the word boundaries and the largest lengths,
    with and without the pop.  The oracle replays the traced actions: every drawn action is in its
    legal set, the last code, flags, return and end reason are its own (a dead end is a state whose
    legal set is exactly the pop), and every final record decodes to its path.  The trace also
    equals the oracle's own draws."""
    P, Ld = _pool(name), _ladder(name)
    seed = SEEDS[name]
    sims = {fwd: _oracle_playouts(name, fwd, seed) for fwd in (False, True)}
    assert _covered(name, sims)
    steps = sims[False]["steps"]
    snap, _, _ = _ladder_snapshots(P, Ld, steps)
    v = _vec(P, 2)
    replays = {}
    for fwd in (False, True):
        out = v.playout(snap, K, L, seed=seed, forward_only=fwd, trace=True, final=True)
        M = sims[fwd]["M"]
        assert len(snap) == M
        trace = out["trace"].cpu().numpy().reshape(L, M * K)
        rep = replays[fwd] = _oracle_playouts(name, fwd, seed, trace=trace)
        for k, key in (("reward_code", "reward_code"), ("flags", "flags"), ("steps", "nsteps"), ("return", "ret"),
                       ("end", "end"), ("first", "first")):
            assert np.array_equal(out[k].cpu().numpy().reshape(-1).astype(np.int64), rep[key]), k
        _same_paths(out["final"], snap.info, P, _view(rep["final"]))
        assert np.array_equal(trace, sims[fwd]["trace"])
    assert _covered(name, replays)
    v.core.sync()


# ----------------------------------------------------------------------------- the deepest records
@pytest.mark.parametrize("name", ["15x15", "16x16"])
def test_restore_and_fork_of_the_deepest_records(on_gpu, name):
    """d. the records of the full snake (225 / 255 points) restored into a fresh context and
    walked back 40 moves, then forked across the batch and walked back 40 more."""
    P, Ld = _pool(name), _ladder(name)
    S, n, pops = Ld["S"], 300, 40
    snap, structs, legal = _ladder_snapshots(P, Ld, [S])
    assert _view(structs)["path_len"].tolist() == [P["points"]] * 2
    back = [a ^ 2 for a in reversed(P["snake"])]
    rng = np.random.default_rng(S)
    first = rng.integers(0, 4, (pops, n)).astype(np.uint8)
    walkers = np.arange(n) % 4 < 2
    first[:, walkers] = np.asarray(back[:pops], np.uint8)[:, None]
    src = np.arange(n) % 2
    v = _vec(P, n)
    _, info = v.restore(snap, src=src)
    assert np.array_equal(info["legal_mask"].cpu().numpy(), legal[src])
    o = COracle(P["opool"], n, True, MAX_STEPS, autoreset=0)
    _copy_envs(o, structs, src)
    ov = _view(o.envs)

    def run(acts):
        assert _families(P["table"], n, len(acts)) == {"k_rollout"}
        out = v.rollout(len(acts), torch.from_numpy(acts).cuda())
        ro, fo = o.rollout(len(acts), acts)
        assert np.array_equal(out["reward_code"].cpu().numpy(), ro) and np.array_equal(out["flags"].cpu().numpy(), fo)
        _same_paths(v.snapshot(), snap.info, P, ov)

    run(first)
    assert (ov["path_len"][walkers] == P["points"] - pops).all()
    fsrc = n - 1 - np.arange(n)
    saved = _save_envs(o)
    v.fork(fsrc)
    _copy_envs(o, saved, fsrc)
    second = rng.integers(0, 4, (pops, n)).astype(np.uint8)
    second[:, walkers[fsrc]] = np.asarray(back[pops:2 * pops], np.uint8)[:, None]
    run(second)
    assert (ov["path_len"][walkers[fsrc]] == P["points"] - 2 * pops).all()
    v.core.sync()
