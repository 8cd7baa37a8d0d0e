"""The exact-fit search of the rule audit on the GPU, on the crafted tilings of tests/tiling_pools.py
(recorded in tests/golden/rules_tilings*.json.gz), along the kernel paths the golden replays do not
reach: the search inside the kernel instead of the region-code table on one-word boards
(cell_mask_p8 + exact_fit + FitMemo), rule rollouts of every kernel with every env and step against
the C oracle (COracle.rollout_rules), the node cap at 1, at a middle value and at its default with
the host finishing what the GPU hands over, and a second audit after the host has answered.

Middle cap: tiling_pools.MID_FIT_CAP = 8, the median node count of the crafted pools' searches as the
CPU harness prints them (tests/test_exact_fit_host.py asserts that it is that median and that at
least ten searches lie on either side of it)."""
import functools

import numpy as np
import pytest

import rules_trace as rt
from golden_io import load
from oracle import COracle, OraclePool, RulesCOracle, rules_ref
from tiling_pools import MID_FIT_CAP

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, T, MAX_STEPS = 520, 24, 60
NO_TABLE = 1      # a region-code table budget (in entries) that no puzzle fits: every region is searched


@functools.lru_cache(maxsize=None)
def _pool(name):
    from sparc_gym_amd.puzzles import process_puzzles
    records = load(name)["records"]
    proc = process_puzzles(records)
    return records, proc, OraclePool(rt.step_pool(proc)), RulesCOracle(proc)


@functools.lru_cache(maxsize=None)
def _trace(name, n=N):
    """The oracle's rule rollout of a crafted pool: env i holds puzzle i mod P for good (no autoreset; a
    pool of even size: (i + i // P) mod P), so every puzzle is held by even and by odd envs;
    even envs walk their puzzle's solution (every third of them part of it), then, like the odd
    ones, random actions.  Read only."""
    records, proc, opool, rules = _pool(name)
    ids = [r["id"] for r in records]
    P = len(proc)
    pids = (np.arange(n) + (np.arange(n) // P if P % 2 == 0 else 0)) % P
    for q in range(len(proc)):                               # each puzzle's solution is walked, twins too
        assert (pids[0::2] == q).any() and (pids[1::2] == q).any(), ids[q]
    acts = rt.actions(proc, pids, T, seed=17)
    o = COracle(opool, n, True, MAX_STEPS, autoreset=0)
    o.reset(pids)
    first = np.array([rules.bits(int(q), [proc[int(q)]["start_location"]], proc[int(q)]["start_location"]) for q in pids],
                     np.int16)
    _, _, bits = o.rollout_rules(T, rules, acts)
    assert (o.state()["pid"] == pids).all()                  # every puzzle is held at every step
    assert (bits >= 0).all() and not (bits & (1 << 9)).any()
    # the pools hold poly / ylop symbols only: the bits that vary are reached_target, poly_ylop_area and all
    assert len(np.unique(bits)) >= 3 and ((bits >> 8) & 1).any() and ((bits >> 7) & 1).any() and not ((bits >> 7) & 1).all()
    for a in (pids, acts, first, bits):
        a.setflags(write=False)
    return pids, acts, first, bits, o.state()


def _vec(name, n=N, **kw):
    from sparc_gym_amd import SPaRCVecEnv
    return SPaRCVecEnv(n, processed=_pool(name)[1], traceback=True, autoreset="none", observation="compact",
                       rules=True, max_steps=MAX_STEPS, **kw)


def _points(vis_words, pitch, X, Y):
    v = sum(int(w) << (64 * k) for k, w in enumerate(vis_words))
    return [[x, y] for x in range(X) for y in range(Y) if (v >> (x * pitch + y)) & 1]


_MAPS = {}


def _oracle_maps(name, vec, st):
    """(region map [n, 64 W], fit mask [n]) of every env's state from oracle/rules_ref.py."""
    proc = _pool(name)[1]
    pitch, words = vec.table.pitch, vec.table.words
    memo, region, fit = _MAPS.setdefault(name, {}), [], []   # the cases of a pool end in the same states
    for i in range(len(st["x"])):
        q = int(st["puzzle"][i])
        key = (q, st["visited"][:, i].tobytes(), int(st["x"][i]), int(st["y"][i]))
        if key not in memo:
            p = proc[q]
            a = rules_ref.RuleAudit(p, _points(st["visited"][:, i], pitch, p["x_size"], p["y_size"]),
                                    (int(st["x"][i]), int(st["y"][i])))
            status, rm = a.validate()
            row = np.full(64 * words, 255, np.uint8)
            for x in range(rm.shape[0]):
                for y in range(rm.shape[1]):
                    if rm[x, y] >= 0:
                        row[x * pitch + y] = rm[x, y]
            mask = sum(1 << int(d["region"]) for d in status["poly_ylop_area"]["detail"].get("region_details", [])
                       if d["ok"])
            memo[key] = (row, mask)
        region.append(memo[key][0])
        fit.append(memo[key][1])
    return np.stack(region), np.array(fit, np.int64)


def test_six_region_puzzles_answer_differently():
    """On the oracle's side: the static regions of the category-h puzzles hold instances and their
    poly / ylop answers differ, so a memo that returned a neighbour's entry would change the bits."""
    for name, rid, least in (("rules_tilings_tb1", "tile-h-six3x3", 6), ("rules_tilings4wg_tb1", "tile-h-strips7x7", 7)):
        records, proc, _, _ = _pool(name)
        p = proc[[r["id"] for r in records].index(rid)]
        det = rules_ref.audit(p, [p["start_location"]], p["start_location"])["poly_ylop_area"]["detail"]["region_details"]
        assert len(det) >= least
        assert {True, False} <= {d["exact_fit"]["ok"] for d in det if d["area_check"]["ok"]}
        assert sum(d["area_check"]["ok"] for d in det) > 4   # more searches per audit than FitMemo holds
        assert rid in [r["id"] for r in records[:N]]          # _trace: every puzzle of a pool is held at every step


CAPS = [1, MID_FIT_CAP, None]
HOST_POOL = "rules_tilings4wg_tb1"     # holds tile-g-host7x7 and its twin: past the GPU's lists, the host's at every cap
KERNELS = [("rules_tilings_tb1", "default"), ("rules_tilings_tb1", "generic"), ("rules_tilings_tb1", "search"),
           ("rules_tilings2w_tb1", "default"), ("rules_tilings4w_tb1", "default"), (HOST_POOL, "default")]


@pytest.mark.parametrize("cap", CAPS, ids=lambda c: f"fit_cap={c}")
@pytest.mark.parametrize("name,kernel", KERNELS)
def test_rule_rollout_and_audits_at_every_cap(on_gpu, name, kernel, cap):
    """Every env and step of a rule rollout, and k_rules / the record audits on the state it leaves,
    against the C oracle; region maps and fit masks against oracle/rules_ref.py.  kernel: the pool's
    default rule rollout (one word: k_rollout1r on the region-code table), the forced generic kernel,
    or `search`: a context without any region-code table, whose audits run cell_mask_p8 and the
    search in the kernel.  Searches past the cap are queued and finished on the host: the outputs are
    the same at every cap, nothing stays unfinished, and a second audit of the same states queues
    nothing (the host's answers are kept)."""
    pids, acts, first, want, _ = _trace(name)
    kw = dict(fit_cap=cap)
    if kernel == "search":
        kw["rule_table_entries"] = NO_TABLE
    vec = _vec(name, **kw)
    if kernel == "generic":
        vec.core.set_variant(vec.core.VARIANT_RULE_ROLLOUT_GENERIC, 1)
    vec.reset(options={"puzzle_index": pids})
    queued = vec.core.rules_queue_stats()["last_searches"]
    assert np.array_equal(vec.rule_audit()["bits"].cpu().numpy(), first)
    r = vec.rollout(T, torch.from_numpy(acts.copy()).cuda(), rules=True)
    queued += vec.core.rules_queue_stats()["last_searches"]
    bits = r["rule_bits"].cpu().numpy()
    assert not (bits & (1 << 9)).any()
    bad = np.argwhere(bits != want)
    assert not len(bad), (len(bad), "first (step, env)", bad[0], bits[tuple(bad[0])], want[tuple(bad[0])])
    st = vec.state()
    region, fit = _oracle_maps(name, vec, st)
    snap = vec.snapshot()
    outs = [vec.rule_audit(region=True, fit=True), vec.audit_records(snap, region=True, fit=True)]
    queued += vec.core.rules_queue_stats()["last_searches"]
    for o in outs:
        assert np.array_equal(o["bits"].cpu().numpy(), want[-1])
        assert np.array_equal(o["region"].cpu().numpy(), region)
        assert np.array_equal(o["fit"].cpu().numpy(), fit)
    assert np.array_equal(vec.audit_records(snap)["bits"].cpu().numpy(), want[-1])   # bits only: table-only kernel
    # the second audit of the same states: the same answers, nothing queued again
    again = vec.rule_audit(region=True, fit=True)
    assert vec.core.rules_queue_stats()["last_searches"] == 0
    assert np.array_equal(again["bits"].cpu().numpy(), want[-1]) and np.array_equal(again["fit"].cpu().numpy(), fit)
    searched = kernel == "search" or name != "rules_tilings_tb1"     # no region-code table for (all of) the pool
    if searched and cap is not None:
        assert queued > 0, "searches past the cap are handed to the host"
    if cap is None:
        assert (queued > 0) == (name == HOST_POOL)           # only the host-only puzzle's searches


def test_host_only_puzzle_and_twin_in_audit_and_rollout(on_gpu):
    """tile-g-host7x7 (more than 16 distinct shapes on 7x7 cells) and its twin through rule_audit and
    one rule rollout at the default cap.  Their solution runs along the board's edge, so the whole
    board stays one region on it: the oracle says that it fits for the one and never for the twin
    (poly_ylop_area, bit 7).  The GPU hands every such search to the host and says the same, in the
    audit's bits and fit mask and for every env and step of the rollout."""
    name = HOST_POOL
    ids = [r["id"] for r in _pool(name)[0]]
    pids, acts, first, want, _ = _trace(name)
    g, twin = pids == ids.index("tile-g-host7x7"), pids == ids.index("tile-g-host7x7-twin")
    assert g.any() and twin.any()
    assert ((first[g] >> 7) & 1).all() and not ((first[twin] >> 7) & 1).any()
    assert ((want[:, g] >> 7) & 1).any() and not ((want[:, twin] >> 7) & 1).any()
    vec = _vec(name)
    vec.reset(options={"puzzle_index": pids})
    queued = vec.core.rules_queue_stats()["last_searches"]
    audit = vec.rule_audit(region=True, fit=True)
    queued += vec.core.rules_queue_stats()["last_searches"]
    assert queued > 0                                        # cap 0 on the GPU: the host's at once
    region, fit = _oracle_maps(name, vec, vec.state())
    assert (fit[g] == 1).all() and (fit[twin] == 0).all()    # one region, number 0
    assert np.array_equal(audit["bits"].cpu().numpy(), first)
    assert np.array_equal(audit["region"].cpu().numpy(), region)
    assert np.array_equal(audit["fit"].cpu().numpy(), fit)
    bits = vec.rollout(T, torch.from_numpy(acts.copy()).cuda(), rules=True)["rule_bits"].cpu().numpy()
    assert not (bits & (1 << 9)).any()
    assert np.array_equal(bits[:, g | twin], want[:, g | twin]) and np.array_equal(bits, want)


def test_middle_cap_queues_some_searches_and_finishes_others(on_gpu):
    """Without a region-code table, over the reset and one rule rollout: the middle cap hands fewer
    searches to the host than cap 1 (some finish on the GPU) and more than none."""
    name = "rules_tilings_tb1"
    pids, acts, _, want, _ = _trace(name)
    queued = {}
    for cap in (1, MID_FIT_CAP):
        vec = _vec(name, fit_cap=cap, rule_table_entries=NO_TABLE)
        vec.core.set_variant(vec.core.VARIANT_HOST_FITS, 1)   # answers not kept: every audit counts its own
        vec.reset(options={"puzzle_index": pids})
        queued[cap] = vec.core.rules_queue_stats()["last_searches"]
        bits = vec.rollout(T, torch.from_numpy(acts.copy()).cuda(), rules=True)["rule_bits"].cpu().numpy()
        queued[cap] += vec.core.rules_queue_stats()["last_searches"]
        assert np.array_equal(bits, want)
    print(queued)
    assert 0 < queued[MID_FIT_CAP] < queued[1]
