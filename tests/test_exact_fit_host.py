"""The exact-fit search (csrc/sparc_rules.hpp exact_fit) on the CPU, under ASan + UBSan.

tests/host/exact_fit_main.cpp is compiled here with -fsanitize=address,undefined and run as a child
process (no GPU, no library, nothing preloaded) on the rule tables the package's own packer makes of
every golden rule pool.  The searches are the distinct (puzzle, region cells) pairs of the pools'
recorded states whose area check passes; the expected answers are oracle/rules_ref.py's own search
(pinned to the reference by the same fixtures), never exact_fit's.  Both instantiations are run: the
GPU's <uint32_t, 16, 16, 6> and the host's <uint64_t, 64, 64, 8>."""
import os
import statistics
import subprocess

import pytest

from golden_io import load
from rules_io import RULE_POOLS, ref_puzzle, snapshots
from sparc_gym_amd.puzzles import pack_rules, pack_table, process_puzzles
from tiling_pools import count_searches

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sparc-gym_amd", "csrc")


@pytest.fixture(scope="module")
def exact_fit_main(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path_factory.mktemp("exact_fit_host") / "exact_fit_main")
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(REPO, "include"), "-I" + CSRC, "-o", exe,
                    os.path.join(REPO, "tests", "host", "exact_fit_main.cpp")], check=True)

    def run(path):
        r = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.splitlines()
    return run


def pool_searches(pool):
    """(records, [(puzzle, cell mask, oracle answer)]) of a golden pool: every distinct search of
    its recorded states, with the oracle's own (uncounted) search as the expected answer."""
    g = load(pool)
    puzzles = [ref_puzzle(p) for p in g["processed"]]
    seen, out = set(), []
    for _, pi, _, s in snapshots(g):
        key = (pi, tuple(map(tuple, s["path"])))
        if key in seen:
            continue
        seen.add(key)
        CY = (puzzles[pi]["y_size"] - 1) // 2
        for srch in count_searches(puzzles[pi], s["path"], s["agent"], count=False):
            rm = sum(1 << ((x - 1) // 2 * CY + (y - 1) // 2) for x, y in srch["cells"])
            if (pi, rm) not in seen:
                seen.add((pi, rm))
                out.append((pi, rm, int(srch["ok"])))
    return g["records"], out


def write_input(path, records, searches):
    proc = process_puzzles(records)
    table = pack_table(proc)
    rt = pack_rules(proc, table)
    with open(path, "w") as f:
        f.write(f"pitch {table.pitch}\npuzzles {len(proc)}\n")
        for q, p in enumerate(proc):
            f.write("%d %d %d %d\n" % ((p["x_size"], p["y_size"]) + rt.inst_range(q)))
        f.write(f"inst {len(rt.inst)}\n" + " ".join(map(str, rt.inst.tolist())) + "\n")
        f.write(f"shapes {len(rt.shape_area)}\n" + " ".join(map(str, rt.shape_first.tolist())) + "\n")
        f.write(f"offsets {len(rt.shape_off)}\n" + " ".join(map(str, rt.shape_off.reshape(-1).tolist())) + "\n")
        f.write(f"searches {len(searches)}\n" + "".join(f"{q} {rm:x}\n" for q, rm, _ in searches))
    return path


def parse(lines):
    out = []
    for ln in lines:
        w = ln.split()
        if w[0] == "S":
            out.append({"q": int(w[1]), "rm": int(w[2], 16), "flagged": int(w[3]), "a32": int(w[4]), "n32": int(w[5]),
                        "a64": int(w[6]), "n64": int(w[7]), "caps": []})
        else:
            out[-1]["caps"].append(tuple(map(int, w[1:])))
    return out


@pytest.mark.parametrize("pool", RULE_POOLS)
def test_exact_fit_both_instantiations_and_caps(exact_fit_main, tmp_path, pool):
    records, searches = pool_searches(pool)
    assert searches
    got = parse(exact_fit_main(write_input(tmp_path / "in.txt", records, searches)))
    assert len(got) == len(searches)
    print(pool, "nodes:", sorted(s["n64"] for s in got))
    for (q, rm, want), s in zip(searches, got):
        where = (pool, records[q]["id"], hex(rm))
        assert (s["q"], s["rm"]) == (q, rm)
        assert s["a64"] == want, where                       # the host's lists and planes, no cap
        if s["flagged"]:                                     # past the GPU's lists: cap 0, "not finished" at once
            assert s["a32"] == -1 and all(r32 == -1 for _, r32, _ in s["caps"]), where
        else:
            assert s["a32"] == want and s["n32"] == s["n64"], where
        assert len(s["caps"]) == 8
        for cap, r32, r64 in s["caps"]:                      # never the opposite answer; finished from its own
            assert r64 == (want if cap >= s["n64"] else -1), (where, cap)   # node count on, at every larger cap
            if not s["flagged"]:
                assert r32 == (want if cap >= s["n32"] else -1), (where, cap)


def test_host_only_puzzle_is_handed_over_at_once_and_answered_on_the_host(exact_fit_main, tmp_path):
    """tile-g-host7x7 (24 polys of 20 distinct shapes on 7x7 cells) and its twin are past the GPU's
    lists: <uint32_t, 16, 16, 6> gets cap 0 and says "not finished" at once, at every cap asked;
    <uint64_t, 64, 64, 8> gives the oracle's answers, fits and does not fit, the first after a search
    of more than a thousand nodes through its 64-entry lists."""
    pool = "rules_tilings4wg_tb1"
    records, searches = pool_searches(pool)
    ids = [r["id"] for r in records]
    got = parse(exact_fit_main(write_input(tmp_path / "in.txt", records, searches)))
    for rid, want in (("tile-g-host7x7", 1), ("tile-g-host7x7-twin", 0)):
        mine = [(srch, s) for srch, s in zip(searches, got) if srch[0] == ids.index(rid)]
        assert len(mine) == 1, rid                           # the whole board, at every recorded state
        (q, rm, oracle), s = mine[0]
        assert rm == (1 << 49) - 1 and oracle == want, rid
        assert s["flagged"] == 1 and s["a32"] == -1 and all(r32 == -1 for _, r32, _ in s["caps"]), rid
        assert s["a64"] == want, rid
        assert all(r64 == (want if cap >= s["n64"] else -1) for cap, _, r64 in s["caps"]), rid
    assert [s["n64"] for (q, _, _), s in zip(searches, got) if q == ids.index("tile-g-host7x7")][0] > 1000
    assert not any(s["flagged"] for (q, _, _), s in zip(searches, got) if not ids[q].startswith("tile-g-"))


def test_middle_fit_cap_is_the_crafted_pools_median(exact_fit_main, tmp_path):
    """tiling_pools.MID_FIT_CAP (the middle node cap of tests/test_gpu_exact_fit.py): the median node count of the crafted pools'
    searches as this harness prints them."""
    nodes = []
    for pool in RULE_POOLS:
        if pool.startswith("rules_tilings"):
            records, searches = pool_searches(pool)
            nodes += [s["n64"] for s in parse(exact_fit_main(write_input(tmp_path / (pool + ".txt"), records, searches)))]
    from tiling_pools import MID_FIT_CAP
    print("searches", len(nodes), "median", statistics.median(nodes), "max", max(nodes))
    assert MID_FIT_CAP == int(statistics.median(nodes))
    assert sum(n > MID_FIT_CAP for n in nodes) >= 10 and sum(n <= MID_FIT_CAP for n in nodes) >= 10
