"""The parts of the record observation that need no GPU: the header's declarations against ``_lib``'s
constants, where ``observe`` is defined, the stream contract of ``SPaRCVecEnv.observe`` on a stub
core, and the argument checks of ``SPaRCVecEnv.observe``, ``SparcCore.observe_records_device`` /
``_host`` and ``search.solution_dataset`` that run before any device call (on objects whose C
context is a stub that fails the test if it is reached)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from sparc_gym_amd import _lib  # noqa: E402
from sparc_gym_amd.core import SparcCore  # noqa: E402
from sparc_gym_amd.search import solution_dataset  # noqa: E402
from sparc_gym_amd.vec_env import OBS_DTYPES, SPaRCVecEnv  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "sparc_gym_amd.h")
X, Y = 7, 5


class _NoDevice:
    """Stands where the C context's binding would: any use fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the check came after a device call ({name})")


class _Snap:
    def __init__(self, M):
        self.M = M

    def __len__(self):
        return self.M


def _vec():
    v = SPaRCVecEnv.__new__(SPaRCVecEnv)
    v.num_puzzles, v.num_envs, v.device, v.core = 12, 4, torch.device("cpu"), _NoDevice()
    v.x_dim, v.y_dim = X, Y
    v._stream = lambda: None
    return v


# ----------------------------------------------------------------------------- the header
def test_header_declares_the_observe_calls_and_the_constants_of_lib():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("sparc_observe_records_device", "sparc_observe_records_host"):
        assert re.search(rf"^int {name}\(void \*ctx, const sparc_snapshot_info \*info, const void \*\w+, int64_t M,\s*"
                         r"const sparc_observe_out \*out\);", src, flags=re.M), name
        assert name in _lib.EXPORTS
    defs = {k: int(v) for k, v in re.findall(r"^#define (SPARC_OBS_\w+) (\d+)$", src, flags=re.M)}
    want = {f"SPARC_{k}": getattr(_lib, k) for k in ("OBS_I32", "OBS_U8", "OBS_F16", "OBS_BF16", "OBS_F32")}
    assert defs == want and sorted(want.values()) == list(range(5))
    assert _lib.OBS_ELEM_BYTES == {_lib.OBS_I32: 4, _lib.OBS_U8: 1, _lib.OBS_F16: 2, _lib.OBS_BF16: 2, _lib.OBS_F32: 4}
    members = re.search(r"typedef struct \{([^}]*)\} sparc_observe_out;", src).group(1)
    assert re.findall(r"(\w+);", members) == [k for k, _ in _lib.SparcObserveOut._fields_]
    assert ctypes.sizeof(_lib.SparcObserveOut) == 64 and _lib.SparcObserveOut.stride.offset == 32
    assert re.search(r"^#define SPARC_ABI_VERSION 2$", src, flags=re.M)
    assert OBS_DTYPES == {torch.int32: _lib.OBS_I32, torch.uint8: _lib.OBS_U8, torch.float16: _lib.OBS_F16,
                          torch.bfloat16: _lib.OBS_BF16, torch.float32: _lib.OBS_F32}
    # the patterns of "one" the header states are the dtypes' own
    for dt, bits in ((torch.float16, 0x3C00), (torch.bfloat16, 0x3F80)):
        assert int(torch.ones(1, dtype=dt).view(torch.int16)[0]) == bits
    assert int(torch.ones(1, dtype=torch.float32).view(torch.int32)[0]) == 0x3F800000
    lib = _lib.load()
    assert lib.sparc_observe_records_device(None, None, None, 1, None) == -1
    assert lib.sparc_observe_records_host(None, None, None, 1, None) == -1


# ----------------------------------------------------------------------------- where observe lives
def test_observe_is_inherited_and_binds_the_stream_before_its_first_core_call():
    """tests/test_stream_binding.py pins the methods defined on SPaRCVecEnv itself; observe comes
    from a base class and keeps the same contract: on an env whose core raises at the first touch,
    _stream() has been called by then, also when an argument check refuses the call."""
    assert callable(getattr(SPaRCVecEnv, "observe")) and "observe" not in vars(SPaRCVecEnv)
    for call in (lambda v: v.observe(_Snap(3)), lambda v: v.observe(_Snap(3), dtype=torch.float16),
                 lambda v: v.observe(_Snap(3), dtype=torch.int64)):
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


# ----------------------------------------------------------------------------- argument checks
def test_observe_refuses_bad_arguments_before_any_device_call():
    v, M = _vec(), 5
    out = torch.zeros((M, 4, X, Y), dtype=torch.int32)
    bad = [
        (dict(snap=_Snap(M), dtype=torch.int64), "dtype"),
        (dict(snap=_Snap(M), dtype=np.int32), "dtype"),
        (dict(snap=_Snap(0)), "records"),
        (dict(snap=_Snap(M), out=out), "together"),
        (dict(snap=_Snap(M), channels=(0, 1)), "together"),
        (dict(snap=_Snap(M), out=np.zeros((M, 4, X, Y), np.int32), channels=(0, 1)), "tensor"),
        (dict(snap=_Snap(M), out=out, channels=(0, 1), dtype=torch.uint8), "dtype"),
        (dict(snap=_Snap(M), out=out.to("meta"), channels=(0, 1)), "device"),
        (dict(snap=_Snap(M + 1), out=out, channels=(0, 1)), "shape"),
        (dict(snap=_Snap(M), out=out[:, :, :, :Y - 1], channels=(0, 1)), "shape"),
        (dict(snap=_Snap(M), out=out[:, 0], channels=(0, 1)), "shape"),
        (dict(snap=_Snap(M), out=out[:, :1], channels=(0, 0)), "shape"),
        (dict(snap=_Snap(M), out=torch.zeros((M, 8, X, Y), dtype=torch.int32)[:, ::2], channels=(0, 1)), "contiguous"),
        (dict(snap=_Snap(M), out=out, channels=(0, 4)), "channels"),
        (dict(snap=_Snap(M), out=out, channels=(-1, 2)), "channels"),
        (dict(snap=_Snap(M), out=out, channels=(2, 2)), "channels"),
        (dict(snap=_Snap(M), out=out, channels=(1,)), "channels"),
        (dict(snap=_Snap(M), out=out, channels=3), "channels"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            v.observe(**kw)
    with pytest.raises(AssertionError, match="device call"):      # and a call within the rules goes on
        v.observe(_Snap(M), out=out, channels=(3, 1))


def _core():
    c = SparcCore.__new__(SparcCore)
    c.lib, c.ctx = _NoDevice(), None
    c.table = types.SimpleNamespace(x_max=X, y_max=Y, words=1)
    return c


def test_observe_records_device_refuses_bad_arguments_before_any_device_call():
    c = _core()
    ok = dict(info=None, d_records=16, M=5, elem=_lib.OBS_F16, x_dim=X, y_dim=Y, stride=0, d_visited=64)
    bad = [
        (dict(elem=5), "elem"),
        (dict(elem=-1), "elem"),
        (dict(M=0), "M must"),
        (dict(M=2**31), "M must"),
        (dict(x_dim=X - 1), "x_dim"),
        (dict(y_dim=Y - 1), "x_dim"),
        (dict(x_dim=16, y_dim=17), "x_dim"),
        (dict(stride=X * Y - 1), "stride"),
        (dict(stride=1), "stride"),
        (dict(stride=-8), "stride"),
        (dict(d_visited=None), "at least one output"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            c.observe_records_device(**{**ok, **kw})
    for kw in (dict(), dict(stride=X * Y), dict(stride=5 * X * Y), dict(x_dim=16, y_dim=16),
               dict(d_visited=None, d_legal=8), dict(x_dim=None, y_dim=None)):
        with pytest.raises(AssertionError, match="device call"):
            c.observe_records_device(**{**ok, **kw})
    info = types.SimpleNamespace(record_bytes=32)
    with pytest.raises(ValueError, match=r"\[M, 32\]"):
        c.observe_records_host(info, np.zeros((4, 48), np.uint8))
    with pytest.raises(ValueError, match="elem"):
        c.observe_records_host(info, np.zeros((4, 32), np.uint8), elem=9)
    with pytest.raises(AssertionError, match="device call"):
        c.observe_records_host(info, np.zeros((4, 32), np.uint8))


def test_solution_dataset_sorts_the_listed_paths_before_any_device_call():
    """Wrong starts and non-unit moves are counted on the host; with nothing left to walk no call
    is made at all, and a puzzle index outside the pool is refused."""
    v = _vec()
    v.puzzles = [
        {"start_location": (0, 0), "solution_paths": [[(1, 0), (2, 0)], [(0, 0), (1, 1)], [(0, 0), (2, 0)]]},
        {"start_location": (2, 2), "solution_paths": [[(2, 2)], [{"x": 2, "y": 3}], [(2, 2), (2, 2)]]},
    ]
    out = solution_dataset(v)
    assert out["skipped"] == {"wrong_start": 2, "non_unit_move": 3, "refused": 0}
    assert out["paths"] == [(1, 0)] and out["visited"] is None and out["action"] is None
    assert solution_dataset(v, [0])["skipped"] == {"wrong_start": 1, "non_unit_move": 2, "refused": 0}
    with pytest.raises(ValueError, match="puzzle_indices"):
        solution_dataset(v, [2])
    v.puzzles[0]["solution_paths"].append([(0, 0), (0, 1)])
    with pytest.raises(AssertionError, match="device call"):      # a path to walk goes on to the core
        solution_dataset(v)
