"""tests/observe_ref.py (the numpy decoder the GPU tests of SPaRCVecEnv.observe lean on) against the
C oracle, without a GPU: the oracle's states after step 20 of the geometry pools' standing trace are
packed into records by hand, bit by bit with Python integers, and decoded; the planes must be the
oracle's own.  One class each of one, two and four words; both traceback modes (the record size and
nothing else differs); plane sizes at and above the table's largest lattice."""
import numpy as np
import pytest

import geometry_pools as gp
import observe_ref

N, T = 320, 24
CLASSES = ("7x7_p8", "w1p4", "w2p7", "7x15_w2p16", "w4p13")


def _pack_by_hand(st, words, pitch, tb):
    """One record per oracle env: pos, step, pid and the board as a little-endian integer."""
    n = len(st["x"])
    rb = observe_ref.record_bytes(words, tb)
    rec = np.zeros((n, rb), np.uint8)
    for i in range(n):
        board = 0
        for x, y in zip(*np.nonzero(st["visited"][i])):
            board |= 1 << (int(x) * pitch + int(y))
        assert board < 1 << (64 * words)
        pos = int(st["x"][i]) | int(st["y"][i]) << 8 | int(st["path_len"][i]) << 16
        head = b"".join(int(v).to_bytes(4, "little") for v in (pos, 0, int(st["step"][i]), int(st["pid"][i])))
        rec[i, :16 + 8 * words] = np.frombuffer(head + board.to_bytes(8 * words, "little"), np.uint8)
    return rec


@pytest.mark.parametrize("tb", [True, False])
@pytest.mark.parametrize("name", CLASSES)
def test_decoder_gives_the_oracles_planes(name, tb):
    table = gp.step_pool(name)[1]
    assert table.words == gp.CLASSES[name]["geom"][0]
    st = gp.step_trace(name, N, T, tb, "next_step")["state20"]
    assert (st["path_len"] > 3).any() and len(np.unique(st["pid"])) > 8
    rec = _pack_by_hand(st, table.words, table.pitch, tb)
    assert rec.shape[1] % 16 == 0
    for xd, yd in ((table.x_max, table.y_max), (table.x_max + 1, table.y_max), (16, 16)):
        vis, agent, pid, loc = observe_ref.decode(rec, table.words, table.pitch, xd, yd)
        assert vis.dtype == np.int32 and vis.shape == (N, xd, yd) == agent.shape
        assert np.array_equal(vis, st["visited"][:, :xd, :yd].astype(np.int32)), (name, tb, xd, yd)
        assert not st["visited"][:, xd:, :].any() and not st["visited"][:, :, yd:].any()
        want = np.zeros((N, xd, yd), np.int32)
        want[np.arange(N), st["x"], st["y"]] = 1
        assert np.array_equal(agent, want) and (agent.sum(axis=(1, 2)) == 1).all()
        assert (vis[np.arange(N), st["x"], st["y"]] == 1).all()        # the agent stands on its path
        assert np.array_equal(pid, st["pid"]) and np.array_equal(loc, np.stack([st["x"], st["y"]], 1))


def test_cells_off_the_board_read_zero():
    """y >= pitch and bits at or above 64 * words are not board bits: a full board of all ones
    decodes to ones on the board only."""
    words, pitch = 1, 4
    rec = np.zeros((1, observe_ref.record_bytes(words, False)), np.uint8)
    rec[0, 16:24] = 0xFF
    vis = observe_ref.decode(rec, words, pitch, 17, 6)[0][0]
    assert vis[:16, :4].all() and not vis[16:].any() and not vis[:, 4:].any()
