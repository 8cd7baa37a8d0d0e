"""sparc_rand_pick (include/sparc_gym_amd.h), the draw of the playouts among the legal actions,
against its numpy twin search.rand_pick: tests/host/rand_pick_main.c includes the header, is
compiled here with the C compiler and run on a few thousand (seed, id, t) with all 16 masks.
No GPU, no library."""
import os
import subprocess

import numpy as np
import pytest

from sparc_gym_amd.search import rand_pick

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096


@pytest.fixture(scope="module")
def picks(tmp_path_factory):
    d = tmp_path_factory.mktemp("rand_pick")
    exe, fin, fout = str(d / "rand_pick_main"), str(d / "in.bin"), str(d / "out.bin")
    subprocess.run([os.environ.get("CC", "gcc"), "-std=c99", "-O1", "-Wall", "-Werror", "-fsanitize=undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(REPO, "include"), "-o", exe,
                    os.path.join(REPO, "tests", "host", "rand_pick_main.c")], check=True)
    rng = np.random.default_rng(7)
    v = rng.integers(0, 2**64, size=(N, 3), dtype=np.uint64)
    # the values the playouts use: small seeds, ids counting up from id0, t a step number; and the extremes
    v[:1024, 0] = rng.integers(0, 100, 1024)
    v[:1024, 1] = np.arange(1024) + 2**32 - 512
    v[:1024, 2] = rng.integers(0, 65535, 1024)
    v[1024] = 0
    v[1025] = 2**64 - 1
    v.astype("<u8").tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr
    return v, np.fromfile(fout, np.uint8).reshape(16, N)


def test_header_equals_the_numpy_twin(picks):
    v, got = picks
    for mask in range(16):
        want = rand_pick(v[:, 0], v[:, 1], v[:, 2], mask)
        assert want.dtype == np.int64 and np.array_equal(got[mask], want), mask
    # broadcasting and plain ints
    assert np.array_equal(rand_pick(5, np.arange(8), 3, 15), [rand_pick(5, i, 3, 15) for i in range(8)])
    assert np.array_equal(rand_pick(v[:, 0], v[:, 1], v[:, 2], 0x35), got[5])        # only bits 0-3 count


@pytest.mark.parametrize("mask", range(16))
def test_only_set_bits_are_drawn_and_each_of_them(picks, mask):
    _, got = picks
    drawn = set(np.unique(got[mask]).tolist())
    want = {d for d in range(4) if (mask >> d) & 1}
    assert drawn == (want or {0})
    if len(want) > 1:          # uniform: each of n bits about N / n times (5 sigma of a binomial)
        n = len(want)
        cnt = np.bincount(got[mask], minlength=4)[sorted(want)]
        assert (np.abs(cnt - N / n) < 5 * np.sqrt(N * (1 / n) * (1 - 1 / n))).all(), cnt


def test_the_draw_is_the_rth_set_bit():
    """r = ((z >> 32) * n) >> 32 with the finaliser of sparc_rand_action: the top two bits of z are
    that function's action, so on the full mask the pick IS sparc_rand_action."""
    z_top = rand_pick(11, np.arange(1000), 4, 15)
    seed, ids, t = np.uint64(11), np.arange(1000, dtype=np.uint64), np.uint64(4)
    with np.errstate(over="ignore"):
        z = seed + ids * np.uint64(0x9E3779B97F4A7C15) + t * np.uint64(0xD1B54A32D192ED03)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    assert np.array_equal(z_top, (z >> np.uint64(62)).astype(np.int64))
