"""The parts of the UCT tree search that need no GPU: the header's declarations against ``_lib``,
where ``mcts`` is defined, the stream contract of ``SPaRCVecEnv.mcts`` on a stub core, the argument
checks of ``SPaRCVecEnv.mcts`` and ``SparcCore.mcts_device`` / ``_host`` that run before any device
call, and the reduction of ``search.uct`` over trees made by the model (tests/mcts_ref.py)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mcts_ref as ref  # noqa: E402
from sparc_gym_amd import _lib, search  # noqa: E402
from sparc_gym_amd.core import SparcCore  # noqa: E402
from sparc_gym_amd.vec_env import SPaRCVecEnv, uct_tables  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "sparc_gym_amd.h")


class _NoDevice:
    """Stands where the C context's binding would: any use fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the check came after a device call ({name})")


class _Snap:
    def __init__(self, M, rb=48):
        self.M = M
        self.info = types.SimpleNamespace(record_bytes=rb)
        self.records = torch.zeros((M, rb), dtype=torch.uint8)

    def __len__(self):
        return self.M


# ----------------------------------------------------------------------------- the header
def test_header_declares_the_mcts_calls_and_the_constants_of_lib():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("sparc_mcts_device", "sparc_mcts_host"):
        assert re.search(rf"^int {name}\(void \*ctx, const sparc_snapshot_info \*info, const void \*\w+, int64_t M,\s*"
                         r"int32_t sims, int32_t L, uint64_t seed, uint64_t id0, uint32_t flags,\s*"
                         r"const float \*\w+, const float \*\w+, int32_t T, int64_t cap, void \*\w+,\s*"
                         r"uint32_t \*\w+, const sparc_mcts_out \*out\);", src, flags=re.M), name
        assert name in _lib.EXPORTS
        args, res = _lib._SIGS[name]
        assert len(args) == 16 and res is ctypes.c_int32 and args[3] is ctypes.c_int64 and args[12] is ctypes.c_int64
    for k, val in (("INVALID", 0), ("DONE", 1), ("FULL", 2), ("PENDING", 3), ("DEAD_END", 4)):
        assert re.search(rf"^#define SPARC_MCTS_{k} {val}$", src, flags=re.M)
        assert getattr(_lib, "MCTS_" + k) == getattr(ref, k) == val
    assert re.search(r"^#define SPARC_MCTS_NODE_BYTES 64$", src, flags=re.M) and _lib.MCTS_NODE_WORDS == 16
    assert re.search(r"^#define SPARC_MCTS_NO_CHILD 0xFFFFFFFFu$", src, flags=re.M)
    assert _lib.MCTS_NO_CHILD == ref.NONE == 0xFFFFFFFF
    assert (_lib.MCTS_VISITS, _lib.MCTS_WINS, _lib.MCTS_LOSSES, _lib.MCTS_CHILD, _lib.MCTS_N, _lib.MCTS_CHILD_WINS) == \
        (ref.VISITS, ref.WINS, ref.LOSSES, ref.CHILD, ref.N, ref.CHILD_WINS)
    members = re.search(r"typedef struct \{([^}]*)\} sparc_mcts_out;", src).group(1)
    names = [n for decl in re.findall(r"([^;]+);", members) for n in re.findall(r"\*?(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [k for k, _ in _lib.SparcMctsOut._fields_]
    assert re.search(r"^#define SPARC_ABI_VERSION 2$", src, flags=re.M)          # additive
    doc = text[text.index("UCT tree search of records"):text.index("#define SPARC_MCTS_INVALID")]
    assert "_get_legal_actions" in doc and "1024-1051" in doc and "1111-1238" in doc and "sparc_rand_pick" in doc
    lib = _lib.load()
    assert lib.sparc_mcts_device(None, None, None, 1, 1, 1, 0, 0, 0, None, None, 2, 1, None, None, None) == -1
    assert lib.sparc_mcts_host(None, None, None, 1, 1, 1, 0, 0, 0, None, None, 2, 1, None, None, None) == -1


# ----------------------------------------------------------------------------- where mcts lives
def _vec():
    v = SPaRCVecEnv.__new__(SPaRCVecEnv)
    v.num_puzzles, v.num_envs, v.device, v.traceback = 12, 4, torch.device("cpu"), True
    v._stream = lambda: None
    return v


def test_mcts_is_inherited_and_binds_the_stream_before_its_first_core_call():
    assert callable(getattr(SPaRCVecEnv, "mcts")) and "mcts" not in vars(SPaRCVecEnv)
    assert [c.__name__ for c in SPaRCVecEnv.__mro__ if "mcts" in vars(c)] == ["_RecordMcts"]
    for call in (lambda v: v.mcts(_Snap(3), 4, 5), lambda v: v.mcts(_Snap(3), 0, 5)):
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


# ----------------------------------------------------------------------------- argument checks
def test_mcts_refuses_bad_arguments_before_any_launch(monkeypatch):
    """Past the header comparison (stubbed: it asks the context), every check precedes the core call."""
    from sparc_gym_amd import snapshot
    monkeypatch.setattr(snapshot, "info_mismatch", lambda a, b: None)
    v = _vec()
    v.core = types.SimpleNamespace(snapshot_info=lambda: None)
    snap = _Snap(3)
    ep, ec = uct_tables()
    nan = ep.copy()
    nan[3] = np.nan
    for kw, what in ((dict(sims=0), "sims"), (dict(sims=2**31), "sims"), (dict(horizon=0), "horizon"),
                     (dict(horizon=65536), "horizon"), (dict(cap=0), "cap"), (dict(cap=2**24 + 1), "cap"),
                     (dict(explore=(nan, ec)), "finite"), (dict(explore=(ep, -np.inf * np.ones_like(ec))), "finite"),
                     (dict(explore=(ep[:5], ec[:6])), "same length"), (dict(explore=(ep[:1], ec[:1])), "T"),
                     (dict(explore=(ep.reshape(2, -1), ec.reshape(2, -1))), "one-dimensional"),
                     (dict(tree={"nodes": torch.zeros((3, 5, 16), dtype=torch.int32)}), "nodes"),
                     (dict(tree={"nodes": torch.zeros((3, 5, 16), dtype=torch.int32).view(torch.uint32)}, cap=4), "cap")):
        args = dict(sims=4, horizon=6)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            v.mcts(snap, **args)
    with pytest.raises(ValueError, match="M must"):
        v.mcts(_Snap(0), 4, 6)
    with pytest.raises(AttributeError, match="mcts_device"):          # and a call within the rules goes on
        v.mcts(snap, 4, 6)
    with pytest.raises(ValueError, match="entries"):
        uct_tables(1.0, 1)


def test_core_checks_precede_the_library():
    c = SparcCore.__new__(SparcCore)
    c.lib, c.ctx = _NoDevice(), None
    ok = dict(info=None, d_records=16, M=5, sims=4, L=6, d_ep=64, d_ec=128, T=8, cap=5, d_nodes=256, d_count=512,
              d_status=8, d_sims_done=8, d_win_rec=16, d_win_steps=8)
    for kw, what in ((dict(M=0), "M must"), (dict(M=2**31), "M must"), (dict(sims=0), "sims"), (dict(L=0), "L "),
                     (dict(L=65536), "L "), (dict(flags=2), "flags"), (dict(T=1), "T "), (dict(cap=0), "cap"),
                     (dict(cap=2**24 + 1), "cap")):
        with pytest.raises(ValueError, match=what):
            c.mcts_device(**{**ok, **kw})
    with pytest.raises(AssertionError, match="device call"):
        c.mcts_device(**ok)
    info = types.SimpleNamespace(record_bytes=32)
    ep, ec = uct_tables(1.0, 8)
    rec = np.zeros((4, 32), np.uint8)
    with pytest.raises(ValueError, match=r"\[M, 32\]"):
        c.mcts_host(info, np.zeros((4, 48), np.uint8), 4, 6, ep, ec, 5)
    with pytest.raises(ValueError, match="same length"):
        c.mcts_host(info, rec, 4, 6, ep, ec[:5], 5)
    with pytest.raises(ValueError, match="nodes"):
        c.mcts_host(info, rec, 4, 6, ep, ec, 5, nodes=np.zeros((4, 5, 16), np.int32))
    with pytest.raises(ValueError, match="win_steps"):
        c.mcts_host(info, rec, 4, 6, ep, ec, 5, win_steps=np.zeros(3, np.uint32))
    with pytest.raises(AssertionError, match="device call"):
        c.mcts_host(info, rec, 4, 6, ep, ec, 5)


def test_default_tables_are_uct_in_float32():
    ep, ec = uct_tables(1.5, 100)
    assert ep.dtype == ec.dtype == np.float32 and ep.shape == ec.shape == (100,)
    assert ep[0] == ep[1] == 0 and ec[0] == ec[1] == 1
    n = np.arange(2, 100)
    assert np.array_equal(ep[2:], (1.5 * np.sqrt(np.log(n.astype(np.float64)))).astype(np.float32))
    assert np.array_equal(ec[2:], (1 / np.sqrt(n.astype(np.float64))).astype(np.float32))
    assert np.allclose(ep[2:] * ec[2:], 1.5 * np.sqrt(np.log(n) / n), rtol=1e-6)


# ----------------------------------------------------------------------------- search.uct on the model's trees
class _Wins:
    def __init__(self, paths):
        self.paths = paths

    def select(self, idx):
        return _Wins([self.paths[int(i)] for i in idx])

    def moves(self):
        return self.paths


class _Rows:
    def __init__(self, rows):
        self.rows = rows

    def __len__(self):
        return len(self.rows)

    def select(self, idx):
        return _Rows([self.rows[int(i)] for i in idx])


def test_uct_sums_the_trees_of_a_root():
    from sparc_gym_amd import synthetic
    from sparc_gym_amd.puzzles import process_puzzles
    pool = [ref.pool_entry(p) for p in process_puzzles(synthetic.make_puzzles(16, seed=0, sizes=((3, 3),)))]
    M, trees, sims, L, cap = 8, 3, 30, 6, 31
    starts = ref.prefixes(pool, M, True, 12, seed=5)
    calls = []

    def mcts(snap, sims, horizon, **kw):
        calls.append(kw)
        rows = snap.rows
        model = ref.search(pool, [starts[j] for j in rows], True, 12, sims, horizon, cap, *ref.uct_tables(kw["c"]),
                           seed=kw["seed"], forward_only=True)
        mcts.model = model
        return {"nodes": torch.from_numpy(np.stack([t.array(cap) for t in model])),
                "count": torch.tensor([len(t.nodes) for t in model], dtype=torch.int32),
                "status": torch.tensor([t.status for t in model], dtype=torch.uint8),
                "sims": torch.tensor([t.sims for t in model], dtype=torch.int32),
                "win": _Wins([list(starts[j][1]) + (t.win_actions or []) for j, t in zip(rows, model)]),
                "win_steps": torch.tensor([-1 if t.win_actions is None else t.win_steps for t in model])}

    vec = types.SimpleNamespace(mcts=mcts, traceback=True)
    out = search.uct(vec, _Rows(list(range(M))), sims, L, c=0.9, trees=trees, seed=4)
    assert calls[0]["seed"] == 4 and calls[0]["tree"] is None and calls[0]["forward_only"] is None
    model = mcts.model
    assert len(model) == M * trees and out["status"].shape == (M, trees)
    assert any(t.status == ref.PENDING for t in model) and any(t.win_actions for t in model)
    for j in range(M):
        mine = model[j * trees:(j + 1) * trees]
        for a in range(4):
            kids = [(t, t.nodes[0][ref.CHILD + a]) for t in mine if t.nodes and t.nodes[0][ref.CHILD + a] not in (0, ref.NONE)]
            assert out["visits"][j, a] == sum(t.nodes[c][ref.VISITS] for t, c in kids)
            assert out["wins"][j, a] == sum(t.nodes[c][ref.WINS] for t, c in kids)
            assert out["losses"][j, a] == sum(t.nodes[c][ref.LOSSES] for t, c in kids)
        if mine[0].status == ref.DONE:
            assert out["visits"][j].sum() == trees * sims
            assert out["best_action"][j] == int(np.argmax(out["visits"][j]))
        else:
            assert out["best_action"][j] == -1 and not out["visits"][j].any()
        won = [t for t in mine if t.win_actions is not None]
        if won:
            best = min(won, key=lambda t: t.win_steps)               # min: the first of the shortest
            assert out["solution"][j] == list(starts[j][1]) + best.win_actions
        else:
            assert out["solution"][j] is None
    with pytest.raises(ValueError, match="tree"):
        search.uct(vec, _Rows([0]), sims, L, trees=0)
