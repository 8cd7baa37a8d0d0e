"""The search helpers of sparc_gym_amd.search on top of SPaRCVecEnv.expand: the compaction of one
level against the oracle's legal masks, and whole legal-move trees against a depth-first walk on
the CPU through the C oracle's step (copied _Env structs), which applies the same rule: expand
the legal actions of states that are not done."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import COracle, _Env
from test_gpu_expand import _S, _composed
from test_gpu_snapshot import N, _tables, _warm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


# ----------------------------------------------------------------------------- 6. one level
@pytest.mark.parametrize("name,tb", [("7x7_full", True), ("mixed_5_11", False)])
def test_expand_frontier_keeps_the_legal_moves_of_live_parents(on_gpu, name, tb):
    from sparc_gym_amd.search import expand_frontier
    S = _S(name, tb)
    v = _warm(S)
    snap = v.snapshot()
    pending = S["state"]["pending"] != 0
    want = [(i, a) for i in range(N) for a in range(4) if (S["legal"][i] >> a) & 1 and not pending[i]]
    assert 0 < len(want) < 4 * (~pending).sum()
    ref = _composed(S, snap)
    rows = np.array([4 * i + a for i, a in want])
    for done in (pending, torch.from_numpy(pending).cuda(), pending.astype(np.uint8) * 2):
        out = expand_frontier(v, snap, done)
        got = list(zip(out["parent"].cpu().tolist(), out["action"].cpu().tolist()))
        assert got == want
        assert np.array_equal(out["children"].records.cpu().numpy(), ref["records"][rows])
        assert np.array_equal(out["reward_code"].cpu().numpy(), ref["code"][rows])
        assert np.array_equal(out["flags"].cpu().numpy(), ref["flags"][rows])
    # by default every parent is live
    out = expand_frontier(v, snap)
    assert len(out["children"]) == sum(bin(int(m)).count("1") for m in S["legal"])
    v.core.sync()


# ----------------------------------------------------------------------------- 7. whole trees
@functools.lru_cache(maxsize=None)
def _walk(name, tb, max_steps, roots, max_depth=None):
    """Depth-first walk of each root's legal-move tree through oracle_step: per root and depth the
    nodes, the children that ended with +100, and those that ended otherwise."""
    _, _, pool = _tables(name)
    o = COracle(pool, 1, tb, max_steps)
    step = o.lib.oracle_step
    step.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                     ctypes.c_void_p]
    code, flags = ctypes.c_int8(), ctypes.c_uint8()
    pc, pf, pp = ctypes.byref(code), ctypes.byref(flags), ctypes.byref(pool.c)
    size = ctypes.sizeof(_Env)
    D = 1 + (max_depth if max_depth is not None else 64)
    nodes, solved, ended = (np.zeros((len(roots), D), np.int64) for _ in range(3))
    for r, q in enumerate(roots):
        o.reset([q])
        root = _Env()
        ctypes.memmove(ctypes.byref(root), ctypes.byref(o.envs[0]), size)
        nodes[r, 0] = 1
        stack = [(root, o.legal(0), 0)]
        while stack:
            env, legal, d = stack.pop()
            if max_depth is not None and d == max_depth:
                continue
            for a in range(4):
                if not (legal >> a) & 1:
                    continue
                child = _Env()
                ctypes.memmove(ctypes.byref(child), ctypes.byref(env), size)
                step(pp, ctypes.byref(child), a, int(tb), max_steps, pc, pf)
                nodes[r, d + 1] += 1
                if flags.value & 3:
                    (solved if code.value == 100 else ended)[r, d + 1] += 1
                else:
                    stack.append((child, (flags.value >> 2) & 15, d + 1))
    depth = int(np.nonzero(nodes.sum(0))[0].max())
    return nodes[:, :depth + 1], solved[:, :depth + 1], ended[:, :depth + 1]


def _enumerate(name, tb, max_steps, roots, max_depth=None, n=None):
    from sparc_gym_amd import SPaRCVecEnv
    from sparc_gym_amd.search import enumerate_paths
    proc, table, _ = _tables(name)
    v = SPaRCVecEnv(len(roots) if n is None else n, processed=proc, table=table, traceback=tb, max_steps=max_steps,
                    autoreset="none", observation="compact")
    out = enumerate_paths(v, roots, max_depth=max_depth)
    v.core.sync()
    return out


def _same_counts(out, ref):
    for key, want in zip(("nodes", "solved", "ended"), ref):
        assert out[key].shape == want.shape, key
        assert np.array_equal(out[key], want), key


def _replay(name, tb, max_steps, q, acts):
    _, _, pool = _tables(name)
    o = COracle(pool, 1, tb, max_steps)
    o.reset([q])
    r, f = o.rollout(len(acts), np.asarray(acts, np.uint8)[:, None])
    return r[:, 0], f[:, 0]


def test_whole_trees_equal_the_cpu_walk(on_gpu):
    roots = tuple(range(64))
    ref = _walk("7x7_full", False, 2000, roots)
    nodes, solved, ended = ref
    # from the oracle's side: neither a trivial nor a runaway pool
    assert 10_000 <= nodes.sum() <= 1_000_000
    assert (solved.sum(1) > 0).any() and (ended.sum(1) > 0).any()
    out = _enumerate("7x7_full", False, 2000, roots)
    _same_counts(out, ref)
    for r, q in enumerate(roots):
        acts = out["solution"][r]
        if solved[r].sum() == 0:
            assert acts is None
            continue
        assert acts is not None and 1 <= len(acts) < nodes.shape[1]
        codes, flags = _replay("7x7_full", False, 2000, q, acts)
        assert codes[-1] == 100 and ((flags[:-1] & 3) == 0).all() and flags[-1] & 3


def test_trees_with_traceback_to_depth_6(on_gpu):
    """Pops make the tree endless: both sides stop at depth 6.  More envs than roots."""
    roots = tuple(range(8))
    ref = _walk("7x7_full", True, 2000, roots, 6)
    assert ref[0].shape[1] == 7 and (ref[0][:, 6] > 0).all()
    _same_counts(_enumerate("7x7_full", True, 2000, roots, max_depth=6, n=11), ref)


# ----------------------------------------------------------------------------- 8. truncation
def test_truncation_inside_a_tree(on_gpu):
    roots = tuple(range(4))
    ref = _walk("7x7_full", False, 10, roots)
    nodes, solved, ended = ref
    assert nodes.shape[1] == 11 and nodes[:, 10].sum() > 0
    assert np.array_equal(solved[:, 10] + ended[:, 10], nodes[:, 10])      # every depth-10 child is done
    out = _enumerate("7x7_full", False, 10, roots)
    _same_counts(out, ref)


def test_frontier_limit(on_gpu):
    from sparc_gym_amd import SPaRCVecEnv
    from sparc_gym_amd.search import enumerate_paths
    proc, table, _ = _tables("7x7_full")
    v = SPaRCVecEnv(4, processed=proc, table=table, traceback=False, max_steps=2000, autoreset="none",
                    observation="compact")
    with pytest.raises(RuntimeError, match="max_frontier"):
        enumerate_paths(v, [0, 1, 2, 3], max_frontier=12)
    with pytest.raises(ValueError):
        enumerate_paths(v, [0, 1, 2, 3, 4])
