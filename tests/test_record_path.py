"""The record path decoder (tests/record_path.py) on records built by hand, without a GPU.

Records of one, two and four words at the lengths where the 2-bit direction stack changes word
(32 moves per 64-bit word) and at the largest length each lattice holds, 255 being the maximum of
the 8-bit length field.  Then the records a decoder must refuse."""
from types import SimpleNamespace

import numpy as np
import pytest

from long_pools import column_snake, row_snake, walk
from record_path import decode, encode

LENGTHS = (1, 2, 32, 33, 34, 64, 65, 66, 128, 129, 225, 255)
# words, pitch, lattice, start: 7x7 padded (49 points), 9x9 (81), 15x15 (225), 16x16 less (0, 0) (255)
SHAPES = {"w1_7x7": (1, 8, 7, (0, 0)), "w2_9x9": (2, 9, 9, (0, 0)), "w4_15x15": (4, 15, 15, (0, 0)),
          "w4_16x16": (4, 16, 16, (0, 1))}


def _info(words, pitch):
    return SimpleNamespace(words=words, pitch=pitch, traceback=1, record_bytes=(16 + 24 * words + 15) // 16 * 16)


def _shape(name):
    words, pitch, X, start = SHAPES[name]
    proc = [{"x_size": X, "y_size": X, "start_location": [9, 9]},          # puzzle 0 is never the record's
            {"x_size": X, "y_size": X, "start_location": list(start)}]
    full = walk(start, column_snake(X, X, start[1]))
    assert len(full) == X * X - start[1] and len(set(full)) == len(full)
    return _info(words, pitch), proc, full


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_length_the_width_holds(name):
    info, proc, full = _shape(name)
    lengths = [n for n in LENGTHS if n <= len(full)]
    if lengths[-1] != len(full):                              # the lattice's maximum is among them
        lengths.append(len(full))
    assert max(lengths) == {"w1_7x7": 49, "w2_9x9": 81, "w4_15x15": 225, "w4_16x16": 255}[name]
    rec = np.stack([encode(info, 1, full[:n], step=7 * n, aux=n, off=n % 3) for n in lengths])
    assert rec.shape == (len(lengths), {1: 48, 2: 64, 4: 112}[info.words])
    got = decode(rec, info, proc)
    for n, g in zip(lengths, got):
        assert g["path"] == full[:n] and g["path_len"] == n and (g["x"], g["y"]) == full[n - 1]
        assert g["visited"] == set(full[:n]) and g["step"] == 7 * n and g["puzzle"] == 1
    # the documented bit positions, restated once without the helper: move k of the record of
    # every length sits at bits 2 (k % 32) of stack word k // 32, after the board words
    W = info.words
    moves = column_snake(*[SHAPES[name][2]] * 2, SHAPES[name][3][1])
    for n, row in zip(lengths, rec):
        stack = row[16 + 8 * W:16 + 24 * W].view("<u8")
        for k in {0, 31, 32, 63, 64, 127, 128, 223, 224, 253} & set(range(n - 1)):
            assert (int(stack[k // 32]) >> (2 * (k % 32))) & 3 == moves[k]
        assert (row[2], row[3]) == (n, n % 3)


def test_stale_fields_above_the_top():
    """Two words: fields above the top are whatever a longer path left, and are ignored.  One
    word: the stored stack is canonical, a set field above the top is an error."""
    info2, proc2, full2 = _shape("w2_9x9")
    for n in (1, 2, 32, 33, 34, 64, 65, 66):
        stale = {k: 1 + k % 3 for k in range(n - 1, 128, 5)}
        assert decode(encode(info2, 1, full2[:n], stale=stale)[None], info2, proc2)[0]["path"] == full2[:n]
    info1, proc1, full1 = _shape("w1_7x7")
    for n, k in ((1, 0), (2, 1), (32, 31), (33, 32), (33, 63), (34, 40)):
        with pytest.raises(AssertionError, match="above the top"):
            decode(encode(info1, 1, full1[:n], stale={k: 2})[None], info1, proc1)


@pytest.mark.parametrize("name", ["w1_7x7", "w2_9x9", "w4_15x15", "w4_16x16"])
def test_inconsistent_records_are_refused(name):
    info, proc, full = _shape(name)
    W = info.words
    n = min(len(full), 130) if W == 4 else len(full) - 3
    good = encode(info, 1, full[:n])
    decode(good[None], info, proc)

    def bad(edit, match):
        r = good.copy()
        edit(r)
        with pytest.raises(AssertionError, match=match):
            decode(r[None], info, proc)

    def flip_move(k):
        def edit(r):
            s = r[16 + 8 * W:16 + 24 * W].view("<u8")
            s[k // 32] ^= np.uint64(1 << (2 * (k % 32)))
        return edit

    def flip_board(pt):
        def edit(r):
            b = pt[0] * info.pitch + pt[1]
            v = r[16:16 + 8 * W].view("<u8")
            v[b // 64] ^= np.uint64(1 << (b % 64))
        return edit

    bad(lambda r: r.__setitem__(0, r[0] ^ 1), "ends at")                 # x
    bad(lambda r: r.__setitem__(2, r[2] - 1), "ends at")                 # one point short
    bad(lambda r: r.__setitem__(2, 0), "length 0")
    for k in sorted({0, 31, 32, 33, 63, 64, 65, 127, 128, n - 2} & set(range(n - 1))):
        bad(flip_move(k), "ends at|twice|leaves|differs")                  # a wrong move in any slot
    bad(flip_board(full[n // 2]), "differs")                              # a path point not on the board
    bad(flip_board(full[n]), "differs")                                   # a visited point off the path
    assert decode(_with(good, flip_board(full[n]))[None], info, proc, allow_extra_visited=True)[0]["path"] == full[:n]
    if info.record_bytes > 16 + 24 * W:                                   # 48-byte records: 8 bytes of padding
        bad(lambda r: r.__setitem__(len(r) - 1, 1), "padding")
    # a path that doubles back onto itself: both the moves and the board are "consistent" otherwise
    loop = full[:5] + [full[3]]
    with pytest.raises(AssertionError, match="twice"):
        decode(encode(info, 1, loop)[None], info, proc)


def _with(row, edit):
    r = row.copy()
    edit(r)
    return r


def test_the_transposed_walk_decodes_too():
    """Moves 0 and 2 at the word boundaries (the column snake there holds 1 and 3 only)."""
    info, proc, _ = _shape("w4_16x16")
    path = walk((0, 1), row_snake(16, 16)[:140])
    assert len(set(path)) == 141 and max(b for _, b in path) == 9
    assert decode(encode(info, 1, path)[None], info, proc)[0]["path"] == path
