"""The rule-audit oracle (oracle/rules_ref.py) against the reference's own rule_status, recorded
per step in tests/golden/rules_*.json.gz."""
import collections

import pytest

from golden_io import load
from oracle import rules_ref
from rules_io import RULE_POOLS, ref_puzzle, snapshots


@pytest.mark.parametrize("pool", RULE_POOLS)
def test_oracle_matches_reference_rule_status(pool):
    g = load(pool)
    puzzles = [ref_puzzle(p) for p in g["processed"]]
    n = 0
    for e, pi, t, s in snapshots(g):
        got = rules_ref.normalize(rules_ref.audit(puzzles[pi], s["path"], s["agent"]))
        assert got == s["rule_status"], (pool, e, t)
        n += 1
    assert n > 50


def test_golden_covers_every_rule_both_ways():
    seen = collections.Counter()
    for pool in RULE_POOLS:
        for *_, s in snapshots(load(pool)):
            for k in rules_ref.RULE_NAMES:
                seen[(k, s["rule_status"][k]["passed"])] += 1
            for d in s["rule_status"]["poly_ylop_area"]["detail"].get("region_details", []):
                seen[("exact_fit", d["exact_fit"]["ok"])] += 1
    for k in rules_ref.RULE_NAMES[2:] + ("exact_fit",):
        assert seen[(k, True)] > 0 and seen[(k, False)] > 0, k


def test_crafted_tilings_cover_the_exact_fit_search():
    """The crafted tiling pools (tests/tiling_pools.py) as recorded in rules_tilings*: per category
    the distinct exact-fit searches whose area check passes, counted with the instrumented oracle on
    the committed fixtures.  Every category answers both ways at least three times (g and h: once);
    the fitting searches of category a undo a poly placement before they succeed; d holds searches
    with one, two and three ylops; f holds every cell grid the code distinguishes, one-word boards
    with and past the region-code table's 12 cells, two- and four-word boards; categories a to e
    each reach a four-word board too; g is the search of more than 16 distinct shapes on 7x7 cells,
    fitting and not; a search on 7x7 cells holds cell (6, 6), bit 48 of the cell mask."""
    import tiling_pools
    names = [p for p in RULE_POOLS if p.startswith("rules_tilings")]
    assert "rules_tilings_tb1" in names and len(names) >= 2
    cov = tiling_pools.coverage([load(p) for p in names])
    print(cov)
    assert sorted(cov) == list("abcdefgh")
    for cat, c in cov.items():
        need = 1 if cat in "gh" else 3
        assert c["fit"] >= need and c["nofit"] >= need, (cat, c)
    assert cov["a"]["fit_undone"] >= 3
    assert cov["d"]["ylops"] == 3 and cov["d"]["ylop_searches"] >= 6
    assert cov["c"]["names"] >= 2
    assert cov["f"]["grids"] >= {(3, 3), (2, 5), (5, 2), (1, 7), (7, 1), (4, 4), (5, 7), (7, 7)}
    assert cov["f"]["cells"] == 49 and cov["f"]["last_cell"]
    for cat in "abcde":
        assert any(7 in grid for grid in cov[cat]["grids"]), cat          # a 15-point lattice side: four words
    assert cov["g"]["names"] >= 17 and cov["g"]["cells"] == 49 and cov["g"]["last_cell"]
    assert cov["g"]["fit_undone"] >= 1 and cov["g"]["nodes"] >= 300       # the fitting search really searches
    assert len(cov["h"]["grids"]) >= 2                                    # six regions on one word and on four
