"""search.monte_carlo's reduction of a playout result (best action, ties, shortest solution), on a
hand-made result dict handed over by a stub vec: no GPU, no library."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from sparc_gym_amd.search import monte_carlo  # noqa: E402


class StubVec:
    traceback = True

    def __init__(self, result):
        self.result, self.calls = result, []

    def playout(self, snap, playouts, horizon, **kw):
        self.calls.append((snap, playouts, horizon, kw))
        return self.result


def _result():
    """3 records x 4 playouts, horizon 5.
    record 0: k0 first 1, 3 steps, +100; k1 first 1, 2 steps, -100; k2 first 3, 2 steps, +100;
              k3 first 3, 2 steps, +100 (the shortest win twice: k2 is the solution)
    record 1: every playout without a step (the record was done)
    record 2: k0 first 0, 5 steps, horizon; k1 first 2, 1 step, -100; k2 first 0, 4 steps, +100;
              k3 first 2, 4 steps, +100 (rates 1/2 and 1/2: the tie goes to action 0)"""
    F = 255
    first = np.array([[1, 1, 3, 3], [F, F, F, F], [0, 2, 0, 2]], np.uint8)
    steps = np.array([[3, 2, 2, 2], [0, 0, 0, 0], [5, 1, 4, 4]], np.int32)
    code = np.array([[100, -100, 100, 100], [0, 0, 0, 0], [1, -100, 100, 100]], np.int8)
    trace = np.full((5, 3, 4), F, np.uint8)
    paths = {(0, 0): [1, 0, 0], (0, 1): [1, 2], (0, 2): [3, 0], (0, 3): [3, 3],
             (2, 0): [0, 1, 0, 1, 0], (2, 1): [2], (2, 2): [0, 3, 3, 0], (2, 3): [2, 1, 1, 0]}
    for (j, k), p in paths.items():
        assert len(p) == steps[j, k] and p[0] == first[j, k]
        trace[:len(p), j, k] = p
    stats = np.zeros((3, 4, 4), np.int32)
    for j in range(3):
        for k in range(4):
            if steps[j, k]:
                stats[j, first[j, k]] += [1, code[j, k] == 100, code[j, k] == -100, steps[j, k]]
    t = torch.from_numpy
    return {"reward_code": t(code), "steps": t(steps), "first": t(first), "trace": t(trace), "stats": t(stats)}, paths


def test_reduction():
    res, paths = _result()
    vec = StubVec(res)
    out = monte_carlo(vec, "SNAP", 4, 5, seed=9)
    (snap, K, L, kw), = vec.calls
    assert (snap, K, L) == ("SNAP", 4, 5) and kw["seed"] == 9 and kw["trace"] and kw["stats"]
    assert kw["forward_only"] is True                        # the default: vec.traceback
    assert np.array_equal(out["visits"], [[0, 2, 0, 2], [0, 0, 0, 0], [2, 0, 2, 0]])
    assert np.array_equal(out["wins"], [[0, 1, 0, 2], [0, 0, 0, 0], [1, 0, 1, 0]])
    assert np.array_equal(out["losses"], [[0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0]])
    assert np.array_equal(out["mean_steps"], [[0, 2.5, 0, 2], [0, 0, 0, 0], [4.5, 0, 2.5, 0]])
    assert out["best_action"].tolist() == [3, -1, 0]         # record 2: 1/2 against 1/2, the lowest action
    assert out["solution"] == [paths[(0, 2)], None, paths[(2, 2)]]   # shortest win, the lowest k among equals


def test_an_unvisited_action_never_beats_a_visited_one_without_wins():
    res, _ = _result()
    res["reward_code"][2] = torch.tensor([1, -100, -100, -100], dtype=torch.int8)
    res["stats"][2, :, 1] = 0
    res["stats"][2, 0, 2], res["stats"][2, 2, 2] = 1, 2
    vec = StubVec(res)
    vec.traceback = False
    out = monte_carlo(vec, "SNAP", 4, 5)
    assert vec.calls[0][3]["forward_only"] is False
    assert out["best_action"].tolist() == [3, -1, 0]         # rate 0 of action 0 beats the unvisited 1
    assert out["solution"][2] is None
    out = monte_carlo(vec, "SNAP", 4, 5, forward_only=True)
    assert vec.calls[1][3]["forward_only"] is True
