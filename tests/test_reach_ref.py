"""tests/reach_ref.py (the breadth-first search the GPU tests of SPaRCVecEnv.reach lean on) without a
GPU: hand-made boards whose answers are written out, and the coverage of the standing record fixture
(the C oracle's states after step 20 of the geometry pools' trace), so that the GPU parity test
cannot pass on an empty case: lost positions, legal moves that lead into one, and a spread of
distances are all there, under both traceback settings."""
import numpy as np
import pytest

import geometry_pools as gp
import reach_ref

N, T = 320, 53
POOLS = ("7x7_p8", "w1p4", "w1p12", "w2p7", "w2p15", "7x15_w2p16", "w4p13")
NONE = reach_ref.NONE


def _puzzle(rows, target):
    """A puzzle from text rows indexed [x][y]: '#' a gap, anything else open."""
    gaps = np.array([[c == "#" for c in r] for r in rows], np.int32)
    return {"x_size": gaps.shape[0], "y_size": gaps.shape[1], "obs_array": {"gaps": gaps}, "target_location": target}


def _visited(shape, points):
    v = np.zeros(shape, np.int32)
    for p in points:
        v[p] = 1
    return v


def test_open_field_is_the_manhattan_distance():
    p = _puzzle(["....", "....", "...."], (2, 3))
    d, ad, live, size, plane = reach_ref.reach_one(p, 0, 0, _visited((3, 4), [(0, 0)]))
    assert (d, live, size) == (5, 0b1001, 11)
    assert ad.tolist() == [5, NONE, NONE, 5]                      # +x and +y lead on, -y and -x leave the lattice
    want = np.array([[abs(2 - x) + abs(3 - y) for y in range(4)] for x in range(3)], np.uint8)
    want[0, 0] = NONE                                             # the agent's point is visited
    assert np.array_equal(plane, want) and plane.dtype == np.uint8


def test_wall_with_one_door():
    p = _puzzle([".....",
                 "###.#",
                 "....."], (2, 0))
    d, ad, live, size, plane = reach_ref.reach_one(p, 0, 0, _visited((3, 5), [(0, 0)]))
    assert (d, live, size) == (8, 0b1000, 10)                     # along row 0 to the door at y = 3, and back
    assert ad.tolist() == [NONE, NONE, NONE, 8]
    assert plane[1].tolist() == [NONE, NONE, NONE, 4, NONE] and plane[0].tolist() == [NONE, 7, 6, 5, 6]
    # the door visited behind the agent's back: lost, the target's side is all that is left of C
    d, ad, live, size, plane = reach_ref.reach_one(p, 0, 0, _visited((3, 5), [(0, 0), (1, 3)]))
    assert (d, live, size) == (NONE, 0, 5) and ad.tolist() == [NONE] * 4
    assert (plane[:2] == NONE).all() and plane[2].tolist() == [0, 1, 2, 3, 4]


def test_agent_on_the_target_and_target_visited():
    p = _puzzle(["...", "...", "..."], (1, 1))
    got = reach_ref.reach_one(p, 1, 1, _visited((3, 3), [(0, 1), (1, 1)]))
    assert got[0] == 0 and got[1].tolist() == [NONE] * 4 and got[2:4] == (0, 0) and (got[4] == NONE).all()
    # a damaged position: the target visited with the agent elsewhere
    got = reach_ref.reach_one(p, 0, 0, _visited((3, 3), [(0, 0), (1, 1)]))
    assert got[0] == NONE and got[2:4] == (0, 0) and (got[4] == NONE).all()


def test_agent_sealed_in_and_a_neighbour_that_is_the_target():
    p = _puzzle(["....", "....", "...."], (2, 3))
    sealed = _visited((3, 4), [(0, 0), (0, 1), (1, 1), (1, 0)])    # the agent back at (0, 0): every neighbour visited
    d, ad, live, size, plane = reach_ref.reach_one(p, 0, 0, sealed)
    assert (d, live, size) == (NONE, 0, 8) and reach_ref.forward_legal(p, 0, 0, sealed) == 0
    d, ad, live, size, plane = reach_ref.reach_one(p, 2, 2, _visited((3, 4), [(2, 2)]))
    assert (d, live) == (1, 0b1110) and ad.tolist() == [NONE, 5, 3, 1]   # +y is the target; -y goes round
    assert plane[2, 3] == 0 and plane[2, 2] == NONE
    # padded planes: cells outside the lattice are 255
    plane = reach_ref.reach_one(p, 2, 2, _visited((3, 4), [(2, 2)]), 5, 6)[4]
    assert plane.shape == (5, 6) and (plane[3:] == NONE).all() and (plane[:, 4:] == NONE).all() and plane[0, 0] == 5


def test_a_legal_move_into_a_dead_pocket_is_not_live():
    p = _puzzle(["...", "...", "..."], (2, 2))
    vis = _visited((3, 3), [(1, 0), (1, 1), (0, 1)])               # the agent at (0, 1): (0, 0) is a pocket
    d, ad, live, size, plane = reach_ref.reach_one(p, 0, 1, vis)
    assert reach_ref.forward_legal(p, 0, 1, vis) == 0b1010 and live == 0b1000 and d == 3
    assert plane[0, 0] == NONE and size == 5


@pytest.mark.parametrize("tb", [False, True])
@pytest.mark.parametrize("name", POOLS)
def test_the_record_fixture_covers_lost_pruned_and_far_positions(name, tb):
    """Floors on state20 of the oracle's trace, for the GPU parity test that runs on the same records:
    at least 4 positions that are lost though not on the target, at least 40 with a forward legal
    action that is not live, at least 14 distinct distances; live is a subset of the forward moves."""
    proc = gp.step_pool(name)[0]
    st = gp.step_trace(name, N, T, tb, "next_step")["state20"]
    r = reach_ref.reach(proc, st["pid"], st["x"], st["y"], st["visited"], 16, 16)
    fwd = np.array([reach_ref.forward_legal(proc[int(q)], x, y, v)
                    for q, x, y, v in zip(st["pid"], st["x"], st["y"], st["visited"])], np.uint8)
    tgt = np.array([tuple(proc[int(q)]["target_location"]) == (int(x), int(y)) for q, x, y in zip(st["pid"], st["x"], st["y"])])
    assert not (r["live"] & ~fwd).any()
    assert np.array_equal(r["dist"] == 0, tgt)
    lost = int(((r["dist"] == NONE) & ~tgt).sum())
    pruned = int(((fwd & ~r["live"]) != 0).sum())
    distinct = len(np.unique(r["dist"]))
    print(f"{name} tb={tb}: lost {lost}, pruned {pruned}, distinct dist {distinct}")
    assert lost >= 4 and pruned >= 40 and distinct >= 14, (name, tb, lost, pruned, distinct)
