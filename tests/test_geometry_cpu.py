"""Every board geometry the packer can choose (tests/geometry_pools.py), on the CPU: the step
machine's model against the C oracle, the host table builders under ASan + UBSan, and the rule
audit's model against the C rule oracle.  tests/test_gpu_geometry.py runs the same classes on the
device; these run first because a CPU failure is cheap."""
import numpy as np
import pytest

import geometry_pools as gp
from kernel_model import KernelModel
from oracle import COracle
from rules_model import audit
from sparc_gym_amd.puzzles import lattice_geometry, pack_rules
from test_tables_host import tables_main, write_pool  # noqa: F401  (tables_main is a fixture)


def test_the_classes_are_the_packers_own_choices():
    """Default classes come out of lattice_geometry unforced; over the 49 single-size pools the
    default packing gives 16 (words, pitch) classes, and DEFAULT plus the standing pools of the
    suite (pitch 8; 9 and 11 on two words; 15 on four) name every one of them."""
    for name, c in gp.DEFAULT.items():
        assert c["pitch"] is None and c["words"] is None
        lat = [{"x_size": 2 * cx + 1, "y_size": 2 * cy + 1} for cx, cy in c["sizes"]]
        pitch, words, x_max, y_max = lattice_geometry(lat)
        assert (words, pitch, x_max, y_max) == c["geom"], name
    seen = set()
    for cx in range(1, 8):
        for cy in range(1, 8):
            pitch, words, _, _ = lattice_geometry([{"x_size": 2 * cx + 1, "y_size": 2 * cy + 1}])
            seen.add((words, pitch))
    assert len(seen) == 16
    standing = {(1, 8), (2, 9), (2, 11), (4, 15)}
    assert seen == standing | {c["geom"][:2] for c in gp.DEFAULT.values()}
    # forced classes: the geometry is not the default one, except the yardstick of each family
    for name, c in gp.FORCED.items():
        table = gp.step_pool(name)[1]
        assert (table.words, table.pitch) == c["geom"][:2], name


def test_families_share_their_puzzles():
    for fam, names in gp.FAMILIES.items():
        procs = [gp.step_pool(k)[0] for k in names] + [gp.rule_pool(k)[0] for k in names[:1]]
        assert all(p is procs[0] for p in procs[:len(names)]), fam
        assert len({gp.CLASSES[k]["geom"][:2] for k in names}) == len(names), fam


@pytest.mark.parametrize("name", list(gp.CLASSES))
@pytest.mark.parametrize("tb", [False, True])
def test_model_matches_oracle_with_chunked_launches(name, tb):
    """tests/kernel_model.py (csrc/sparc_env.hpp restated) equals the oracle on every class, with
    the launch cut at arbitrary points so the state round-trips through its stored form."""
    proc, table, opool = gp.step_pool(name)
    n, T, max_steps = 24, 96, 40
    pids = gp.puzzle_indices(n, len(proc))
    acts = gp.actions(name, n, T)
    for autoreset in (1, 0):
        m = KernelModel(table, n, tb, max_steps, autoreset)
        m.reset(pids)
        cuts = [0, 1, 2, 5, 13, 40, 41, T]
        parts = [m.rollout(acts[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        o = COracle(opool, n, tb, max_steps, autoreset)
        o.reset(pids)
        ro, fo = o.rollout(T, acts)
        assert not m.guard_fired
        assert np.array_equal(np.concatenate([p[0] for p in parts]), ro), autoreset
        assert np.array_equal(np.concatenate([p[1] for p in parts]), fo), autoreset
        assert (ro == 100).any() and ((fo & 3) != 0).any()


def test_table_builders_on_every_class(tables_main, tmp_path):  # noqa: F811
    """The puzzle and rule table builders under ASan + UBSan on every class, with and without the
    move stack; the harness re-derives every table entry and is told which branch each class is
    meant to reach (split_w, tab_all, ring_ok)."""
    dirs = []
    for name, c in gp.CLASSES.items():
        proc, table = gp.rule_pool(name)[:2]
        rules = pack_rules(proc, table)
        expect = dict(expect_split_w=c["split_w"], expect_tab_all=c["tab_all"])
        expect["expect_ring_ok"] = c["ring_ok"] or 0            # never on multi-word boards
        rooted = ((table.info[:, 1] >> 16) & 2) != 0
        expect["expect_wide"] = int((rooted & ((table.info[:, 3] & 0xFFFF) > 127)).any())   # a trie of 8-B records
        for tb_on in (1, 0):
            dirs.append(write_pool(tmp_path / f"{name}_tb{tb_on}", table, rules, traceback=tb_on, **expect))
    assert tables_main("check", *dirs) == [f"ok {d}" for d in dirs]


def test_expect_ring_ok_is_checked(tables_main, tmp_path):  # noqa: F811
    """The harness refuses a pool that does not reach the ring_ok branch the test names."""
    proc, table = gp.rule_pool("w1p4")[:2]
    d = write_pool(tmp_path / "w1p4_wrong", table, pack_rules(proc, table), expect_ring_ok=1)
    with pytest.raises(AssertionError, match="ring_ok"):
        tables_main("check", d)


def test_w1p4_reaches_the_generic_rule_rollout_by_itself():
    """k_rollout1r needs ring_ok (x_size * pitch <= 57 for every puzzle); w1p4's 15x3 lattices at
    pitch 4 fill all 64 bits, so its rule rollout is the generic kernel's without any variant.
    test_table_builders_on_every_class checks the loader's ring_ok against this table."""
    c = gp.CLASSES["w1p4"]
    proc, table = gp.rule_pool("w1p4")[:2]
    assert c["ring_ok"] == 0 and table.words == 1 and c["tab_all"] == 1
    assert max(int(p["x_size"]) for p in proc) * table.pitch == 60 > 57
    assert [k for k in gp.DEFAULT if gp.DEFAULT[k]["ring_ok"] == 0] == ["w1p4"]


def _env_path(e):
    return [[e.path[k][0], e.path[k][1]] for k in range(e.path_len)]


@pytest.mark.parametrize("name", list(gp.CLASSES))
def test_rules_model_matches_c_oracle(name):
    """tests/rules_model.py (csrc/sparc_rules.hpp restated, pitch a parameter) against the C rule
    oracle on 192 states of the oracle's own trace per class: 4 envs after each of 48 steps, the
    reset steps of the autoreset among them."""
    proc, table, opool, rules = gp.rule_pool(name)
    rt = pack_rules(proc, table)
    n, T = 64, 48
    acts = gp.actions(name, n, T, rule=True)
    o = COracle(opool, n, True, 24, autoreset=1)
    o.reset(gp.puzzle_indices(n, len(proc)))
    rng = np.random.default_rng(13)
    checked = passed = 0
    for t in range(T):
        _, _, bits = o.rollout_rules(1, rules, acts[t:t + 1], t0=t)
        for i in rng.choice(n, size=4, replace=False):
            e = o.envs[i]
            vis = 0
            for x, y in _env_path(e):
                vis |= 1 << (x * table.pitch + y)
            got, _, rmap = audit(rt, table, e.pid, vis, e.x, e.y)
            assert got == int(bits[0, i]) == rules.bits(e.pid, _env_path(e), (e.x, e.y)), (t, i)
            X, Y = proc[e.pid]["x_size"], proc[e.pid]["y_size"]
            assert set(rmap) == {x * table.pitch + y for x in range(1, X, 2) for y in range(1, Y, 2)}, (t, i)
            checked += 1
            passed += (got >> 8) & 1
    assert checked == 192
