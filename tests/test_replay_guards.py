"""The parts of the replay feature that need no GPU: ``search.actions_from_points`` on the golden
pool's own solution lists, the argument checks of ``SPaRCVecEnv.replay`` and
``SparcCore.replay_device`` that run before any device call (on objects whose C context is a stub
that fails the test if it is reached), and the header's declarations against ``_lib``'s constants."""
import os
import re

import numpy as np
import pytest

import golden_io

torch = pytest.importorskip("torch")

from sparc_gym_amd import _lib  # noqa: E402
from sparc_gym_amd.core import SparcCore  # noqa: E402
from sparc_gym_amd.search import actions_from_points, score_paths  # noqa: E402
from sparc_gym_amd.vec_env import SPaRCVecEnv  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "sparc_gym_amd.h")
MOVES = ((1, 0), (0, -1), (-1, 0), (0, 1))   # right, up, left, down (dir_dx / dir_dy, sparc_env.hpp)


def _walk(start, acts):
    pts = [tuple(start)]
    for a in acts:
        pts.append((pts[-1][0] + MOVES[a][0], pts[-1][1] + MOVES[a][1]))
    return pts


# ----------------------------------------------------------------------------- actions_from_points
def test_every_listed_solution_of_poolA_round_trips():
    g = golden_io.load("poolA_tb1")
    seen = 0
    for p in g["processed"]:
        for sol in p["solution_paths"]:
            acts, ok = actions_from_points(p["start"], sol)
            assert ok and acts.dtype == np.uint8 and len(acts) == len(sol) - 1
            assert ((acts >= 0) & (acts <= 3)).all()
            assert _walk(p["start"], acts.tolist()) == [tuple(pt) for pt in sol]
            as_dicts, ok2 = actions_from_points(tuple(p["start"]), [{"x": x, "y": y} for x, y in sol])
            assert ok2 and np.array_equal(as_dicts, acts)
            seen += 1
    assert seen >= len(g["processed"])   # every puzzle of the pool lists a solution


def test_a_diagonal_a_jump_and_a_repeat_are_255_at_their_index():
    pts = [(2, 6), (2, 5), (3, 4), (3, 3), (3, 1), (3, 1), (2, 1)]
    acts, ok = actions_from_points((2, 6), pts)
    assert ok and acts.tolist() == [1, 255, 1, 255, 255, 2]


def test_a_wrong_first_point_is_reported():
    acts, ok = actions_from_points((0, 0), [(2, 6), (2, 5)])
    assert not ok and acts.tolist() == [1]
    for pts in ([], [(0, 0)]):
        acts, ok = actions_from_points((0, 0), pts)
        assert ok and len(acts) == 0 and acts.dtype == np.uint8
    assert not actions_from_points((0, 0), [(1, 0)])[1]


# ----------------------------------------------------------------------------- argument checks
class _NoDevice:
    """Stands where the C context's binding would: any use fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the check came after a device call ({name})")


def _vec(P=12):
    v = SPaRCVecEnv.__new__(SPaRCVecEnv)
    v.num_puzzles, v.num_envs, v.device, v.core = P, 4, torch.device("cpu"), _NoDevice()
    v._stream = lambda: None
    return v


def test_replay_and_roots_bind_the_stream_before_their_first_core_call():
    """The contract tests/test_stream_binding.py checks for the methods defined on SPaRCVecEnv
    itself, for the two of its base class: on an env whose core raises at the first touch, _stream()
    has been called by then, also when an argument check refuses the call."""
    assert {"replay", "roots"} <= {k for k in dir(SPaRCVecEnv) if callable(getattr(SPaRCVecEnv, k))}
    for call in (lambda v: v.replay(puzzle_indices=[0, 1], actions=np.zeros((2, 2), np.uint8)),
                 lambda v: v.roots([0, 1]), lambda v: v.replay()):
        events = []

        class Core:
            def __getattr__(self, k):
                events.append("core." + k)
                raise RuntimeError(k)

        v = _vec()
        v.core = Core()
        v._stream = lambda: events.append("_stream")
        with pytest.raises((RuntimeError, ValueError)):
            call(v)
        assert events and events[0] == "_stream", events
    assert events == ["_stream"]                    # the refused call never reached the core



def _core():
    c = SparcCore.__new__(SparcCore)
    c.lib, c.ctx = _NoDevice(), None
    return c


class _Snap:
    def __init__(self, M):
        self.M = M

    def __len__(self):
        return self.M


def test_replay_refuses_bad_arguments_before_any_device_call():
    v, M = _vec(), 5
    acts = np.zeros((3, M), np.uint8)
    q = np.arange(M)
    bad = [
        (dict(), "exactly one"),
        (dict(snap=_Snap(M), puzzle_indices=q, actions=acts), "exactly one"),
        (dict(snap=_Snap(0), actions=acts), "start states"),
        (dict(puzzle_indices=np.zeros((2, 2), np.int64), actions=acts), "start states"),
        (dict(puzzle_indices=q, actions=acts.astype(np.int64)), "uint8"),
        (dict(puzzle_indices=q, actions=torch.zeros((3, M), dtype=torch.int32)), "uint8"),
        (dict(puzzle_indices=q, actions=[[0] * M]), "numpy array or tensor"),
        (dict(puzzle_indices=q, actions=np.zeros((3, M + 1), np.uint8)), "shape"),
        (dict(puzzle_indices=q, actions=np.zeros(M, np.uint8)), "shape"),
        (dict(puzzle_indices=q, actions=np.zeros((0, M), np.uint8)), "1..65535"),
        (dict(puzzle_indices=q, actions=np.zeros((65536, M), np.uint8)), "1..65535"),
        (dict(puzzle_indices=q, actions=acts, lengths=np.full(M, 4)), "lengths"),
        (dict(puzzle_indices=q, actions=acts, lengths=np.full(M, -1)), "lengths"),
        (dict(puzzle_indices=q, actions=acts, lengths=np.zeros(M + 1, np.int64)), "lengths"),
        (dict(puzzle_indices=q, actions=acts, lengths=np.zeros(M)), "lengths"),
        (dict(puzzle_indices=q, actions=acts, lengths=torch.zeros(M)), "lengths"),
        (dict(puzzle_indices=q, lengths=np.zeros(M, np.int64)), "without actions"),
        (dict(puzzle_indices=q, per_step=True), "without actions"),
        (dict(puzzle_indices=q, states=True), "without actions"),
        (dict(puzzle_indices=np.array([0, 12]), actions=acts[:, :2]), "puzzle_indices"),
        (dict(puzzle_indices=np.array([-1, 0]), actions=acts[:, :2]), "puzzle_indices"),
        (dict(puzzle_indices=np.array([0.5, 1.0]), actions=acts[:, :2]), "puzzle_indices"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            v.replay(**kw)
    with pytest.raises(ValueError, match="puzzle_indices"):
        v.roots([12])
    with pytest.raises(ValueError, match="same number"):
        score_paths(v, [0, 1], [[0]])
    with pytest.raises(ValueError, match="0..255"):
        score_paths(v, [0], [[0, 256]])


def test_replay_device_refuses_bad_arguments_before_any_device_call():
    c = _core()
    ok = dict(info=None, d_records=16, d_puzzle=None, M=5, L=3, d_actions=32, d_end=48)
    bad = [
        (dict(d_puzzle=64), "exactly one"),
        (dict(d_records=None), "exactly one"),
        (dict(M=0), "M must"),
        (dict(M=2**31), "M must"),
        (dict(L=-1), "L must"),
        (dict(L=65536), "L must"),
        (dict(flags=4), "flags"),
        (dict(flags=1 | 1 << 31), "flags"),
        (dict(L=0), "L = 0"),
        (dict(L=0, d_actions=None, d_step_code=64), "L = 0"),
        (dict(L=0, d_actions=None, d_states=64), "L = 0"),
        (dict(d_actions=None), "actions"),
        (dict(d_end=None), "at least one output"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            c.replay_device(**{**ok, **kw})
    with pytest.raises(AssertionError, match="device call"):      # and a call within the rules goes on
        c.replay_device(**ok)
    with pytest.raises(ValueError, match=r"\[L, M\]"):
        c.replay_host(None, np.zeros(4, np.uint8), puzzle=np.zeros(4, np.uint32))


# ----------------------------------------------------------------------------- the GPU test's inputs
def _standing_cases():
    from test_gpu_replay import FLAGS, MODES, STANDING
    return [(n, tb, m, sd, si) for n, tb in STANDING for m in MODES for sd, si in FLAGS]


@pytest.mark.parametrize("name,tb,mode,stop_done,stop_illegal", _standing_cases())
def test_guard_the_standing_sequences_reach_every_end_reason(name, tb, mode, stop_done, stop_illegal):
    """What tests/test_gpu_replay.py asserts on its chained yardstick before it looks at the kernel,
    here on the C oracle alone: the drawn action strings give every end reason their flag
    combination can produce, a sequence without a step and one of L steps, and (next-step
    autoreset, no STOP_DONE) sequences that run on into the next puzzle."""
    import test_gpu_replay as t
    S = t._S(name, tb)
    acts, lens = t.standing_actions(name, tb)
    assert set(np.unique(acts).tolist()) == {0, 1, 2, 3, 4, 255} and lens.min() == 0 and lens.max() == t.L2
    r = t.oracle_replay(S, mode, acts, lens, stop_done, stop_illegal)
    assert set(np.unique(r["end"]).tolist()) == t._possible(stop_done, stop_illegal)
    assert (r["steps"] == 0).any() and (r["steps"] == t.L2).any()
    if mode == "next_step" and not stop_done:
        assert (r["step_flags"] & 64).any()
    took = np.arange(t.L2)[:, None] < r["steps"][None, :]
    assert not r["step_code"][~took].any() and not r["step_flags"][~took].any()
    assert np.array_equal(r["return"], r["step_code"].sum(0))
    if stop_illegal:                                    # actions above 3 are refused like any illegal one
        refused = r["end"] == _lib.REPLAY_END_ILLEGAL
        a_bad = acts[np.minimum(r["bad"], t.L2 - 1), np.arange(len(lens))][refused]
        assert (a_bad >= 4).any() and (a_bad < 4).any()


# ----------------------------------------------------------------------------- the header
def test_header_declares_the_replay_calls_and_the_constants_of_lib():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("sparc_replay_device", "sparc_replay_host"):
        assert re.search(rf"^int {name}\(void \*ctx, const sparc_snapshot_info \*info,", src, flags=re.M), name
        assert name in _lib.EXPORTS
    defs = {k: int(v.rstrip("u")) for k, v in re.findall(r"^#define (SPARC_REPLAY_\w+) (\d+u?)$", src, flags=re.M)}
    want = {f"SPARC_{k}": getattr(_lib, k) for k in dir(_lib) if k.startswith("REPLAY_")}
    assert defs == want and len(want) == 8
    members = re.search(r"typedef struct \{([^}]*)\} sparc_replay_out;", src).group(1)
    assert re.findall(r"\*(\w+);", members) == [k for k, _ in _lib.SparcReplayOut._fields_]
    assert _lib.load().sparc_replay_device(None, None, None, None, 1, 0, None, None, 0, None) == -1
    assert _lib.load().sparc_replay_host(None, None, None, None, 1, 0, None, None, 0, None) == -1
