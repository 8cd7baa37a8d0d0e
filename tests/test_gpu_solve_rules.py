"""search.solve_by_rules against an exhaustive walk on the CPU: every self-avoiding path from the
start to the target of a puzzle, enumerated depth-first in pure Python on the processed puzzle
(lattice, gaps, start, target) and audited by oracle/rules_ref.py, against the GPU's breadth-first
walk (expand_frontier) and its records audit (audit_records)."""
import numpy as np
import pytest

from oracle import rules_ref

torch = pytest.importorskip("torch")

DIRS = {0: (1, 0), 1: (0, -1), 2: (-1, 0), 3: (0, 1)}    # SPaRC_Gym.py:212-217
SEED, COUNT, SIZES = 6, 8, ((2, 2), (3, 3))               # 5 x 5 and 7 x 7 lattices
RULE_ALL = 1 << 8


def pool():
    from sparc_gym_amd import synthetic
    from sparc_gym_amd.puzzles import process_puzzles
    return process_puzzles(synthetic.make_rule_puzzles(COUNT, seed=SEED, sizes=SIZES, break_prob=0.3))


def cpu_paths(p):
    """{action tuple: (rule bits, listed)} of every self-avoiding start-to-target path of processed
    puzzle p: a move enters a lattice point that is no gap and not on the path (_get_legal_actions,
    SPaRC_Gym.py:1024-1051, without the traceback pop), and the walk ends on the target (1192)."""
    X, Y = p["x_size"], p["y_size"]
    gaps = np.asarray(p["obs_array"]["gaps"])
    start, target = tuple(int(v) for v in p["start_location"]), tuple(int(v) for v in p["target_location"])
    assert start != target
    listed = {tuple(tuple(int(c) for c in pt) for pt in sp) for sp in p["solution_paths"][:p["solution_count"]]}
    ref = dict(p)
    out = {}
    path, acts, on = [start], [], {start}

    def walk():
        x, y = path[-1]
        if (x, y) == target:
            status = rules_ref.audit(ref, [list(pt) for pt in path], (x, y))
            out[tuple(acts)] = (rules_ref.rule_bits(status), tuple(path) in listed)
            return
        for a, (dx, dy) in DIRS.items():
            nx, ny = x + dx, y + dy
            if 0 <= nx < X and 0 <= ny < Y and gaps[nx, ny] == 0 and (nx, ny) not in on:
                path.append((nx, ny)), acts.append(a), on.add((nx, ny))
                walk()
                path.pop(), acts.pop(), on.remove((nx, ny))

    walk()
    return out


@pytest.fixture(scope="module")
def reference():
    """The CPU side, computed once: per puzzle its paths with bits and membership in the solution
    list.  The seed is chosen so that the comparison cannot be empty or one-sided."""
    proc = pool()
    want = [cpu_paths(p) for p in proc]
    assert {(p["x_size"], p["y_size"]) for p in proc} == {(5, 5), (7, 7)}
    assert all(len(w) >= 1 for w in want)                                          # every puzzle has a path
    assert any(b & RULE_ALL for w in want for b, _ in w.values())                  # a satisfied path
    assert any(not b & RULE_ALL for w in want for b, _ in w.values())              # an unsatisfied one
    assert any(ls for w in want for _, ls in w.values())
    return proc, want


def test_reference_side_is_not_empty(reference):
    """The seed's properties, checked without a GPU."""
    proc, want = reference
    assert len(want) == COUNT and sum(len(w) for w in want) > 100


@pytest.mark.gpu
def test_solve_by_rules_equals_the_exhaustive_walk(on_gpu, reference):
    from sparc_gym_amd import SPaRCVecEnv, search
    proc, want = reference
    runs = {}
    for tb in (True, False):
        vec = SPaRCVecEnv(COUNT, processed=proc, traceback=tb, autoreset="none", observation="compact", max_steps=64)
        res = search.solve_by_rules(vec, np.arange(COUNT))
        vec.core.sync()
        runs[tb] = res
        for r in range(COUNT):
            got = {tuple(a): (int(b), bool(s), bool(ls)) for a, b, s, ls in
                   zip(res["paths"][r], res["bits"][r], res["satisfied"][r], res["listed"][r])}
            assert len(got) == len(res["paths"][r])                                # no path twice
            assert set(got) == set(want[r]), (tb, r)
            for a, (bits, listed) in want[r].items():
                assert got[a] == (bits, bool(bits & RULE_ALL), listed), (tb, r, a)
            depth = [len(a) for a in res["paths"][r]]
            assert depth == sorted(depth)                                          # ascending depth
            assert res["nodes"][r, 0] == 1 and res["nodes"][r].sum() >= len(got)
    for k in ("paths",):                                                           # the pops change nothing
        assert runs[True][k] == runs[False][k]
    for k in ("bits", "satisfied", "listed"):
        for r in range(COUNT):
            assert np.array_equal(runs[True][k][r], runs[False][k][r]), (k, r)
    assert np.array_equal(runs[True]["nodes"], runs[False]["nodes"])


@pytest.mark.gpu
def test_max_steps_below_the_lattice_is_refused(on_gpu, reference):
    from sparc_gym_amd import SPaRCVecEnv, search
    proc, _ = reference
    vec = SPaRCVecEnv(COUNT, processed=proc, traceback=True, autoreset="none", observation="compact", max_steps=48)
    with pytest.raises(ValueError, match="max_steps"):
        search.solve_by_rules(vec, np.arange(COUNT))                               # 7 x 7: 49 points
    small = [q for q, p in enumerate(proc) if p["x_size"] * p["y_size"] == 25]
    res = search.solve_by_rules(vec, small)                                        # 5 x 5 alone: 25 <= 48
    assert all(len(p) >= 1 for p in res["paths"])
