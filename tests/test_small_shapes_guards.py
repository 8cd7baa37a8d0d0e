"""CPU guards of tests/test_gpu_small_shapes.py: on tests/small_shapes.py and the oracle alone.

What the GPU tests rely on is asserted here without a GPU: that every case's launches run the kernel
the case is named for (the dispatch conditions of rollout_impl, restated in small_shapes.families),
that its launch lengths and env counts walk the branches the kernel has, and that the ORACLE's trace
of the case holds what the comparison needs (terminated, truncated and illegal steps, autoresets
across launch boundaries, rule-bit patterns) at every env count, env 0 alone included."""
import numpy as np
import pytest

import small_shapes as ss

SPLIT = ("k_rollout1s", "k_rolloutWs")
FALLBACK = {"k_rollout1s": "k_rollout1", "k_rolloutWs": "k_rollout"}
IDS = [c["id"] for c in ss.CASES]


def _fams(c, n, T):
    P = ss.pool(c["pool"])
    return ss.families(P.table, n, T, given=c["given"], obs=c["obs"], rules=c["rules"], variant=c["variant"])


def _runs_kernel(c, n):
    """whether a batch of n envs reaches the case's kernel at all (the split kernels: whole
    256-env workgroups only)"""
    return c["kernel"] not in SPLIT or n % 256 == 0


def test_the_lists():
    for L in (16, 15, 12, 10, 4):
        Ts = ss.launch_lengths(L)
        assert set(Ts) >= {1, 2, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 3 * L, 3 * L + 1, 4 * L, 4 * L + 1, 5 * L,
                           5 * L + 3}
        assert len(set(Ts)) == len(Ts)
    assert 6 * 16 in ss.launch_lengths(16, "k_rollout1")                     # past the ring of 4 tiles
    for G, A, RT in ss.R1R_SHAPES.values():                                  # past the three reward / flag buffers
        assert {6 * RT, 6 * RT + 1} <= set(ss.launch_lengths(RT, "k_rollout1r"))
    for E in (64, 128, 256):
        ns = ss.env_counts(E)
        assert set(ns) == {1, 2, 3, 15, 16, 17, 48, 63, 64, 65, 80, E - 16, E - 1, E, E + 1, E + 16, 2 * E}
        assert list(ns) == sorted(set(ns))
        assert set(ss.trimmed_counts(E)) == {1, 17, 63, 64, 65, E - 1, E, E + 1, E + 16}
    assert {256, 512} <= set(ss.SPLIT_COUNTS) and sum(n % 256 != 0 for n in ss.SPLIT_COUNTS) == 2


def test_the_table_of_cases():
    """Every row of the issue's table is there, with the settings it asks for."""
    def have(kernel, **kw):
        return [c for c in ss.CASES if c["kernel"] == kernel and all(c[k] == v for k, v in kw.items())]
    both = ({False, True}, {"next_step", "none"})
    for kernel, pool in (("k_rollout1", "7x7_full"), ("k_rollout1", "w1p10"), ("k_rollout1s", "7x7_full"),
                         ("k_rolloutWs", "mixed_5_11")):
        cs = have(kernel, pool=pool)
        assert ({c["tb"] for c in cs}, {c["autoreset"] for c in cs}) == both, (kernel, pool)
    for kernel in ("k_rollout1", "k_rollout1s", "k_rolloutWs", "k_rollout", "k_rollout_obsw", "k_rollout_obs",
                   "k_rollout1r", "k_rollout_rules"):
        assert have(kernel, given=False), f"{kernel}: no case with drawn actions"
        assert {c["tb"] for c in have(kernel)} == {False, True}, kernel
    assert have("k_rollout1s", variant={"IO_CODES_OFF": 1})
    for name in ("mixed_5_11", "15x15"):
        assert have("k_rolloutWs", pool=name) and have("k_rollout", pool=name)
    for name in ("7x7_full", "mixed_5_11", "15x15"):
        assert {c["tb"] for c in have("k_rollout_obsw", pool=name)} == {False, True}
        assert have("k_rollout_obs", pool=name, variant={"OBS_INLINE": 1})
    assert {c["variant"].get("R1R_SHAPE", 0) for c in have("k_rollout1r", pool="A")} == {0, 1, 2, 3, 4, 5}
    assert have("k_rollout1r", pool="B") and have("k_rollout1r", pool="A", autoreset="none")
    for name in ("A", "C", "D"):
        assert have("k_rollout_rules", pool=name)
    for c in ss.CASES:
        assert 12 <= c["max_steps"] <= 24 and len(ss.pool(c["pool"]).proc) <= 64
        trimmed = c["pool"] == "D" or c["variant"].get("OBS_INLINE") or c["variant"].get("R1R_SHAPE")
        if c["kernel"] in SPLIT:
            assert c["ns"] == ss.SPLIT_COUNTS
        elif c["pool"] == "w1p10":
            assert c["ns"] == (256, 512)
        elif trimmed:
            assert c["ns"] == ss.trimmed_counts(c["E"])
        else:
            assert set(c["ns"]) == {n for n in ss.env_counts(c["E"])
                                    if c["kernel"] not in ("k_rollout1", "k_rollout") or n % 256}
    geo = ss.pool("w1p10").table
    assert geo.words == 1 and not 3 <= geo.pitch <= 9
    assert [ss.pool(n).table.words for n in ("7x7_full", "mixed_5_11", "15x15", "A", "B", "C", "D")] == [1, 2, 4, 1, 1, 2, 4]


@pytest.mark.parametrize("cid", IDS)
def test_dispatch_and_tile_counts(cid):
    """Every launch of the case runs the kernel it is named for (a split kernel hands its T % 16 tail
    to the fallback kernel, and runs whole 256-env batches only), and over the launches that kernel
    sees 0 to 5 full tiles, a short last tile and an exactly full one: on the tiled pipeline at some
    env count, where the kernel has per-step paths beside it."""
    c = ss.CASE[cid]
    piped_somewhere = False
    for n in c["ns"]:
        per_launch = [_fams(c, n, T) for T in c["Ts"]]
        if not _runs_kernel(c, n):
            assert all([f["kernel"] for f in fs] == [FALLBACK[c["kernel"]]] for fs in per_launch), (cid, n)
            continue
        mine = []
        for T, fs in zip(c["Ts"], per_launch):
            names = [f["kernel"] for f in fs]
            if c["kernel"] in SPLIT:
                want = ([c["kernel"]] if T >= 16 else []) + ([FALLBACK[c["kernel"]]] if T % 16 else [])
                assert names == want, (cid, n, T, names)
                assert sum(f["steps"] for f in fs) == T
                if T >= 16:
                    assert fs[0]["PR"] == (1 if c["kernel"] == "k_rollout1s" and c["given"] else 4)
                    assert fs[0]["IOR"] == (not c["variant"].get("IO_CODES_OFF"))
                    assert fs[0]["short"] == 0 and fs[0]["full_tiles"] == T // 16
                    mine.append((T // 16, T % 16))            # the tail it hands over
            else:
                assert names == [c["kernel"]], (cid, n, T, names)
                f = fs[0]
                assert (f["L"], f["E"]) == (c["L"], c["E"]) and f["steps"] == T, (cid, f)
                assert f["last_wg_full"] == (n % c["E"] == 0) and f["tiled"] == (n % 16 == 0)
                if f["piped"] or c["kernel"] in ("k_rollout1r", "k_rollout_obsw"):
                    mine.append((f["full_tiles"], f["short"]))
                else:
                    assert (f["full_tiles"], f["short"]) == (0, T)    # per-step paths only
        if not mine:
            continue
        piped_somewhere = True
        lo = 1 if c["kernel"] in SPLIT else 0                 # a split kernel never runs without a tile
        assert {k for k, _ in mine} >= set(range(lo, 6)), (cid, n, mine)
        assert any(k >= 1 and s > 0 for k, s in mine) and any(k >= 1 and s == 0 for k, s in mine), (cid, n, mine)
        assert any(k == 0 and s > 0 for k, s in mine) or c["kernel"] in SPLIT
        if c["kernel"] not in ("k_rollout", "k_rollout_obs", "k_rollout_rules"):   # (one tile buffer per wave there)
            assert max(k for k, _ in mine) >= 6               # past every ring and buffer count
    assert piped_somewhere, cid


# the grids every kernel is run on; the split kernels take whole workgroups only, and a whole
# 256-env batch of a pool that reaches them leaves the generic k_rollout only their tails
GRIDS = {"below_a_wave", "one_wave", "partial_workgroup", "full_workgroup", "full_plus_1", "full_plus_16"}


@pytest.mark.parametrize("kernel", sorted({c["kernel"] for c in ss.CASES}))
def test_grids_of_each_kernel(kernel):
    seen = set()
    for c in ss.CASES:
        if c["kernel"] == kernel:
            got = {ss.shape_class(n, c["E"]) for n in c["ns"] if _runs_kernel(c, n)}
            if kernel not in SPLIT + ("k_rollout1", "k_rollout"):
                assert got >= GRIDS, (c["id"], got)              # in every case, the trimmed lists too
            seen |= got
    want = {"full_workgroup", "more"} if kernel in SPLIT else GRIDS - ({"full_workgroup"} if kernel == "k_rollout" else set())
    assert seen >= want, (kernel, seen)


@pytest.mark.parametrize("cid", IDS)
def test_floors_on_the_oracles_trace(cid):
    """At every env count of the case the oracle's cumulative trace holds a terminated step, a
    truncated one and an illegal action; under next-step autoreset an autoreset taken as a launch's
    first step and a done step as a launch's last; in rule cases two rule-bit patterns and, where the
    pool has a puzzle whose listed solution passes every rule, an all-pass state."""
    c = ss.CASE[cid]
    tr = ss.trace(cid)
    assert tr.n == max(c["ns"]) and [l["T"] for l in tr.launches] == list(c["Ts"])
    for n in c["ns"]:
        ss.assert_floors(c, tr, n)
    if c["given"]:
        assert {0, 1, 2, 3, 4, 255} == set(np.unique(tr.acts).tolist())
    if c["rules"]:
        assert ss.pool(c["pool"]).allpass                        # pools A-D all hold such a puzzle


def test_a_batch_is_the_first_columns_of_the_trace():
    """What lets one trace serve every env count: the oracle's trace of n envs equals the first n
    columns of the trace at the largest count (given and drawn actions, rules)."""
    for cid in ("k_rollout1-7x7_full-tb1-next_step-drawn", "k_rollout1r-A-tb1-none-given"):
        c = ss.CASE[cid]
        big = ss.trace(cid)
        for n in (1, 17):
            small = ss._trace(c, n)
            for a, b in zip(small.launches, big.launches):
                for k in ("rew", "flags", "bits", "stats"):
                    if a[k] is not None:
                        assert np.array_equal(a[k], b[k][..., :n] if k != "stats" else b[k][:n]), (cid, n, k)
            for k, v in small.state.items():
                assert np.array_equal(v, big.state[k][:n]), (cid, n, k)
