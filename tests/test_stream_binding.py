"""Every public method of SPaRCVecEnv that touches the device binds the caller's current stream before
its first call into the core.  Checked without a GPU, on an env whose core raises at the first touch;
tests/test_gpu_streams.py checks on a GPU that the stream bound afterwards is the current one."""
from unittest import mock

import pytest

torch = pytest.importorskip("torch")

from test_gpu_streams import PUBLIC  # noqa: E402


class _Touched(Exception):
    pass


@pytest.mark.parametrize("method", PUBLIC)
def test_every_public_method_binds_before_its_first_core_call(method):
    """Without a GPU: on an env whose core raises at the first touch, _stream() has been called by
    then.  (has_state is a plain attribute of the core, not a call.)"""
    from sparc_gym_amd import SPaRCVecEnv
    assert sorted(PUBLIC) == sorted(k for k, f in vars(SPaRCVecEnv).items()
                                    if callable(f) and not k.startswith("_") and k != "close")
    events = []

    class Core:
        has_state = True

        def __getattr__(self, k):
            events.append("core." + k)
            raise _Touched(k)

    v = object.__new__(SPaRCVecEnv)
    v.core, v.device, v.num_envs, v.num_puzzles, v.traceback, v.rules = Core(), torch.device("cpu"), 4, 2, True, False
    v._rbits = torch.zeros(4, dtype=torch.int16)
    v._stream = lambda: events.append("_stream")
    arg = mock.MagicMock()
    args = {"step": (arg,), "rollout": (3,), "random_actions": (3,), "restore": (arg,), "fork": (arg,),
            "playout": (arg, 1, 2), "audit_records": (arg,), "dfs": (arg, 5)}.get(method, ())
    try:
        getattr(v, method)(*args)
    except (_Touched, TypeError, ValueError, RuntimeError):   # the stub core, or an argument check on the mock
        pass
    assert events and events[0] == "_stream", (method, events)
