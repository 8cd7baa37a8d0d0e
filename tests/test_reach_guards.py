"""The parts of the record reachability that need no GPU: the header's declarations against
``_lib``, where ``reach`` is defined, the stream contract of ``SPaRCVecEnv.reach`` on a stub core,
and the argument checks of ``SPaRCVecEnv.reach`` and ``SparcCore.reach_records_device`` / ``_host``
that run before any device call (on objects whose C context is a stub that fails the test if it is
reached)."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sparc_gym_amd  # noqa: E402
from sparc_gym_amd import _lib, search  # noqa: E402
from sparc_gym_amd.core import SparcCore  # noqa: E402
from sparc_gym_amd.vec_env import REACH_NONE, SPaRCVecEnv  # noqa: E402

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
def test_header_declares_the_reach_calls_and_the_constant_of_lib():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("sparc_reach_records_device", "sparc_reach_records_host"):
        assert re.search(rf"^int {name}\(void \*ctx, const sparc_snapshot_info \*info, const void \*\w+, int64_t M,\s*"
                         r"const sparc_reach_out \*out\);", src, flags=re.M), name
        assert name in _lib.EXPORTS
    assert re.search(r"^#define SPARC_REACH_NONE 255$", src, flags=re.M)
    assert _lib.REACH_NONE == REACH_NONE == sparc_gym_amd.REACH_NONE == 255
    members = re.search(r"typedef struct \{([^}]*)\} sparc_reach_out;", src).group(1)
    names = [n for decl in re.findall(r"([^;]+);", members) for n in re.findall(r"\*?(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [k for k, _ in _lib.SparcReachOut._fields_]
    assert ctypes.sizeof(_lib.SparcReachOut) == 48 and _lib.SparcReachOut.x_dim.offset == 40
    assert re.search(r"^#define SPARC_ABI_VERSION 2$", src, flags=re.M)
    # the comment says what a forward move is, and what is out of scope
    doc = text[text.index("target reachability"):text.index("#define SPARC_REACH_NONE")]
    assert "_get_legal_actions" in doc and "1024-1051" in doc and "no counterpart" in doc and "strided" in doc
    lib = _lib.load()
    assert lib.sparc_reach_records_device(None, None, None, 1, None) == -1
    assert lib.sparc_reach_records_host(None, None, None, 1, None) == -1


# ----------------------------------------------------------------------------- where reach lives
def test_reach_is_inherited_and_binds_the_stream_before_its_first_core_call():
    """reach comes from a base class of its own and keeps the contract of the methods defined on
    SPaRCVecEnv itself: on an env whose core raises at the first touch, _stream() has been called by
    then, also when an argument check refuses the call."""
    assert callable(getattr(SPaRCVecEnv, "reach")) and "reach" not in vars(SPaRCVecEnv)
    assert [c.__name__ for c in SPaRCVecEnv.__mro__ if "reach" in vars(c)] == ["_RecordReach"]
    for call in (lambda v: v.reach(_Snap(3)), lambda v: v.reach(_Snap(3), plane=True), lambda v: v.reach(_Snap(0))):
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
def test_reach_refuses_an_empty_snapshot_before_any_device_call():
    v = _vec()
    with pytest.raises(ValueError, match="records"):
        v.reach(_Snap(0))
    with pytest.raises(AssertionError, match="device call"):      # and a call within the rules goes on
        v.reach(_Snap(5), plane=True)


def _core():
    c = SparcCore.__new__(SparcCore)
    c.lib, c.ctx = _NoDevice(), None
    c.table = types.SimpleNamespace(x_max=X, y_max=Y, words=1)
    return c


def test_reach_records_device_refuses_bad_arguments_before_any_device_call():
    c = _core()
    ok = dict(info=None, d_records=16, M=5, x_dim=X, y_dim=Y, d_plane=64)
    bad = [
        (dict(M=0), "M must"),
        (dict(M=2**31), "M must"),
        (dict(x_dim=X - 1), "x_dim"),
        (dict(y_dim=Y - 1), "x_dim"),
        (dict(x_dim=16, y_dim=17), "x_dim"),
        (dict(d_plane=None), "at least one output"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            c.reach_records_device(**{**ok, **kw})
    # the plane's size is read only with a plane
    for kw in (dict(), dict(x_dim=16, y_dim=16), dict(x_dim=None, y_dim=None), dict(d_plane=None, d_dist=8),
               dict(d_plane=None, d_live=8, x_dim=1, y_dim=1), dict(d_plane=None, d_action_dist=8, d_size=8)):
        with pytest.raises(AssertionError, match="device call"):
            c.reach_records_device(**{**ok, **kw})
    info = types.SimpleNamespace(record_bytes=32)
    with pytest.raises(ValueError, match=r"\[M, 32\]"):
        c.reach_records_host(info, np.zeros((4, 48), np.uint8))
    with pytest.raises(ValueError, match=r"\[M, 32\]"):
        c.reach_records_host(info, np.zeros((0, 32), np.uint8))
    with pytest.raises(ValueError, match="x_dim"):
        c.reach_records_host(info, np.zeros((4, 32), np.uint8), x_dim=X - 1)
    with pytest.raises(AssertionError, match="device call"):
        c.reach_records_host(info, np.zeros((4, 32), np.uint8), plane=False, x_dim=1)


def test_the_search_helpers_take_prune_and_default_to_todays_walk():
    for f in (search.expand_frontier, search.solve_by_rules):
        p = inspect.signature(f).parameters["prune"]
        assert p.default is False
    for f in (search.monte_carlo, search.enumerate_paths, search.solve_dfs):
        assert "prune" not in inspect.signature(f).parameters
