"""The host table builders (csrc/sparc_tables.hpp) on the CPU, under ASan + UBSan.

tests/host/tables_main.cpp includes only the two host-side headers, is compiled here with
-fsanitize=address,undefined and run as a child process on pools packed by the package's own
packers.  It derives every expected table entry from the input tables alone; this file chooses
the pools (one per branch of the builders) and holds the rejection texts.  No GPU, no library."""
import os
import subprocess

import numpy as np
import pytest

from sparc_gym_amd import synthetic
from sparc_gym_amd.puzzles import lattice_geometry, pack_rules, pack_table, process_puzzles

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sparc-gym_amd", "csrc")
INVALID = -1   # SPARC_E_INVALID


@pytest.fixture(scope="module")
def tables_main(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path_factory.mktemp("tables_host") / "tables_main")
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-O1", "-g", "-Wall",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + rocm_include,
                    "-I" + os.path.join(REPO, "include"), "-I" + CSRC, "-o", exe,
                    os.path.join(REPO, "tests", "host", "tables_main.cpp")], check=True)

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.splitlines()
    return run


def write_pool(path, table, rules=None, absent=(), **meta):
    """The raw arrays and meta.txt of one pool; `absent` arrays are not written (null pointers)."""
    os.makedirs(path)
    m = dict(words=table.words, pitch=table.pitch, traceback=1, num_puzzles=len(table.info), num_nodes=len(table.trie))
    arrays = dict(open=table.open, info=table.info, trie=table.trie)
    if rules is not None:
        m.update(rules=1, num_inst=len(rules.inst), num_shapes=len(rules.shape_area), num_offsets=len(rules.shape_off))
        arrays.update(planes=rules.planes, inst_first=rules.inst_first, inst=rules.inst, shape_first=rules.shape_first,
                      shape_area=rules.shape_area, shape_off=rules.shape_off)
    m.update(meta)
    for name, a in arrays.items():
        if name not in absent:
            np.ascontiguousarray(a).tofile(os.path.join(path, name + ".bin"))
    with open(os.path.join(path, "meta.txt"), "w") as f:
        f.writelines(f"{k} {int(v)}\n" for k, v in m.items())
    return path


def _pool(n, seed, cells, **kw):
    recs = synthetic.make_rule_puzzles(n // 2, seed=seed, sizes=((cells, cells),), break_prob=0.3)
    recs += synthetic.make_puzzles(n - n // 2, seed=seed + 1, sizes=((cells, cells),), full_properties=True, max_shaped=4)
    proc = process_puzzles(recs)
    table = pack_table(proc, **kw)
    return proc, table, pack_rules(proc, table)


@pytest.fixture(scope="module")
def pool7():
    return _pool(16, 3, 3)


@pytest.fixture(scope="module")
def pool15():
    return _pool(8, 7, 7, pitch=15, words=4)


def _copy(t):
    return type(t)(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vars(t).items()})


def test_puzzle_and_rule_tables_of_every_branch(tables_main, tmp_path, pool7, pool15):
    proc7, t7, r7 = pool7
    dirs = [write_pool(tmp_path / "w1", t7, r7)]
    # the region-code table's budget ends inside the pool: 512 entries per 9-cell puzzle
    dirs.append(write_pool(tmp_path / "w1_budget", t7, r7, reg_entries=5 * 512 + 100, expect_tab_all=0))
    # one cell's net area past 8 bits
    big = _copy(r7)
    big.shape_area[big.inst[0] >> 11] = 200
    dirs.append(write_pool(tmp_path / "w1_area", t7, big, expect_area_ok=0))
    # a puzzle without solutions: no root, no trie records
    bare = [dict(p) for p in proc7]
    bare[5]["solution_count"], bare[5]["solution_paths"] = 0, []
    tb = pack_table(bare)
    assert not (tb.info[5, 1] >> 16) & 2
    dirs.append(write_pool(tmp_path / "w1_rootless", tb, pack_rules(bare, tb), expect_rootless=1))
    # one trie past 127 nodes (8-B records in the mixed table) beside compact ones
    rng = np.random.default_rng(11)
    wide = process_puzzles([synthetic.make_puzzle(rng, 3, 3, n_solutions=48, shared_prefix_prob=0.1, full_properties=False)]
                           + synthetic.make_puzzles(3, seed=12, sizes=((3, 3),), full_properties=False))
    tw = pack_table(wide)
    assert (tw.info[:, 3] > 127).sum() == 1
    dirs.append(write_pool(tmp_path / "w1_wide", tw, expect_wide=1))
    # multi-word pools: the split geometry with and without the move stack, and pitch 16
    _, t11, r11 = _pool(8, 5, 5)
    assert (t11.words, t11.pitch) == (2, 11)
    _, t15, r15 = pool15
    for name, t, r in (("w2", t11, r11), ("w4", t15, r15)):
        for tb_on in (1, 0):
            dirs.append(write_pool(tmp_path / f"{name}_tb{tb_on}", t, r, traceback=tb_on, expect_split_w=1, expect_tab_all=0))
    _, t16, r16 = _pool(4, 9, 7, pitch=16, words=4)
    dirs.append(write_pool(tmp_path / "w4_pitch16", t16, r16, expect_split_w=0, expect_tab_all=0))
    # puzzles past the GPU search's lists: 17 ylops; 16 ylops + 16 shapes (not past); 17 shapes
    cells = [x * 15 + y for x in range(1, 15, 2) for y in range(1, 15, 2)]
    ylop = lambda k: cells[k] | (1 << 10)                     # noqa: E731  (shape 0)
    poly = lambda k, c: cells[c] | (k << 11)                  # noqa: E731
    lists = [[ylop(k) for k in range(17)], [ylop(k) for k in range(16)] + [poly(k, 16 + k) for k in range(16)],
             [poly(k, k) for k in range(17)]] + [[] for _ in range(len(t15.info) - 3)]
    hf = _copy(r15)
    hf.inst = np.asarray(sum(lists, []), np.uint32)
    hf.inst_first = np.cumsum([0] + [len(v) for v in lists]).astype(np.uint32)
    hf.shape_first = np.arange(18, dtype=np.uint32)
    hf.shape_area = np.ones(17, np.int32)
    hf.shape_off = np.zeros((17, 2), np.int8)
    dirs.append(write_pool(tmp_path / "w4_hostfit", t15, hf, expect_split_w=1, expect_tab_all=0, expect_host_fit=2))
    out = tables_main("check", *dirs)
    assert out == [f"ok {d}" for d in dirs]


def test_hostfits_mirror_and_hot_set(tables_main):
    assert tables_main("hostfits") == ["ok hostfits"]


def test_every_rejection_keeps_its_code_and_text(tables_main, tmp_path, pool7, pool15):
    """One table per rejection of the two loaders, corrupted in that one field; the texts are the
    loaders' from before the builders were split out."""
    _, t7, r7 = pool7
    _, t15, r15 = pool15
    assert t7.pitch == 8 and len(r7.inst) >= 10 and len(r7.shape_area) >= 1
    rooted = int(np.flatnonzero((t7.info[:, 1] >> 16) & 2)[1])
    base, cnt = int(t7.info[rooted, 2]), int(t7.info[rooted, 3])
    assert cnt >= 2
    cases = []

    def case(text, table=t7, rules=None, edit=None, **kw):
        t, r = _copy(table), _copy(rules) if rules is not None else None
        if edit:
            edit(t, r)
        cases.append((write_pool(tmp_path / f"case{len(cases)}", t, r, **kw), text))

    def setw(arr, idx, val):
        arr[idx] = val

    case("null argument", absent=("open",))
    case("empty puzzle table", num_puzzles=0)
    case("bad trie", num_nodes=-1)
    case("bad trie", absent=("trie",))
    case("puzzle 2: lattice 9x7 does not fit pitch 8 / 1 words (words=1 needs the padded layout)",
         edit=lambda t, r: setw(t.info, (2, 0), (int(t.info[2, 0]) & ~0xFF) | 9))
    case("puzzle 1: lattice 15x16 does not fit pitch 15 / 4 words", table=t15,
         edit=lambda t, r: setw(t.info, (1, 0), (int(t.info[1, 0]) & ~0xFF00) | (16 << 8)))
    case("puzzle 0: start/target outside the lattice",
         edit=lambda t, r: setw(t.info, (0, 0), (int(t.info[0, 0]) & ~0xFF0000) | (7 << 16)))
    case(f"puzzle {rooted}: trie range out of bounds", edit=lambda t, r: setw(t.info, (rooted, 3), len(t.trie) + 1))
    case("trie child out of range", edit=lambda t, r: setw(t.trie, (base, 0), (int(t.trie[base, 0]) & ~0xFFFF) | cnt))
    case("trie parent out of range",
         edit=lambda t, r: setw(t.trie, (base + 1, 2), (int(t.trie[base + 1, 2]) & ~0xFFFF) | cnt))
    case("null argument", rules=r7, absent=("planes",))
    case("null argument", rules=r7, null_rules=1)
    case("rule table puzzle count differs from the loaded puzzle table", rules=r7, rule_puzzles=len(t7.info) - 1)
    case("bad rule table sizes", rules=r7, num_inst=-1)
    case("bad rule table sizes", rules=r7, absent=("shape_area",))
    case("shape offsets must start at 0", rules=r7, edit=lambda t, r: setw(r.shape_first, 0, 1))
    case("shape offsets out of range", rules=r7, edit=lambda t, r: setw(r.shape_first, 1, len(r.shape_off) + 1))
    case("instance offsets must start at 0", rules=r7, edit=lambda t, r: setw(r.inst_first, 0, 1))
    case("puzzle 0: the rule audit supports lattices up to 15x15", table=t15, rules=r15,
         edit=lambda t, r: setw(t.info, (0, 0), (int(t.info[0, 0]) & ~0xFF) | 17))
    case("instance range out of bounds", rules=r7, edit=lambda t, r: setw(r.inst_first, len(t.info), len(r.inst) + 1))
    case("puzzle 0: 10 instances on 9 cells", rules=r7,
         edit=lambda t, r: setw(r.inst_first, slice(1, None), np.maximum(r.inst_first[1:], 10)))
    case("bad instance", rules=r7,
         edit=lambda t, r: setw(r.inst, 0, (int(r.inst[0]) & 0x7FF) | (len(r.shape_area) << 11)))
    out = tables_main("reject", *[d for d, _ in cases])
    assert out == [f"{INVALID}|{text}" for _, text in cases]


def test_a_path_holds_at_most_255_points(tables_main, tmp_path):
    """The path length is an 8-bit field of the state and of a snapshot record, so both loaders
    refuse a puzzle whose path could hold 256 points: the gap-free 16x16 lattice, the one shape
    the 256-bit board holds and the length does not.  One closed point makes it legal."""
    from long_pools import square_pool
    with pytest.raises(ValueError, match="255 points"):
        pack_table(square_pool(16, closed=False))
    with pytest.raises(ValueError, match="256 bits.*255 points"):      # past the board: the rule, not "15x15 max"
        lattice_geometry([{"x_size": 17, "y_size": 17}])
    t255 = pack_table(square_pool(16, closed=True))
    assert (t255.words, t255.pitch) == (4, 16)
    assert sum(bin(int(w)).count("1") for w in t255.open[0]) == 255
    t225 = pack_table(square_pool(15, closed=False))
    assert (t225.words, t225.pitch) == (4, 15)
    assert sum(bin(int(w)).count("1") for w in t225.open[0]) == 225
    t81 = pack_table(square_pool(9, closed=False))
    assert (t81.words, t81.pitch) == (2, 9)
    # pitch 16 never reaches the multi-word split kernel; the gap-free 9x9 and 15x15 tables do
    ok = [write_pool(tmp_path / "p255", t255, expect_split_w=0), write_pool(tmp_path / "p225", t225, expect_split_w=1),
          write_pool(tmp_path / "p81", t81, expect_split_w=1)]
    assert tables_main("check", *ok) == [f"ok {d}" for d in ok]
    # the same table with point (0, 0) of puzzle 2 opened: 256 open points
    t256 = _copy(t255)
    t256.open[2, 0] |= np.uint64(1)
    # and with the start of puzzle 1 moved onto the closed point: 255 open points and the start
    tstart = _copy(t255)
    tstart.info[1, 0] = int(tstart.info[1, 0]) & 0x0000FFFF
    bad = [write_pool(tmp_path / "p256", t256), write_pool(tmp_path / "pstart", tstart)]
    assert tables_main("reject", *bad) == [
        f"{INVALID}|puzzle 2: a path could hold 256 points, at most 255 fit (8-bit path length)",
        f"{INVALID}|puzzle 1: a path could hold 256 points, at most 255 fit (8-bit path length)"]
