"""The rule audit of state records (k_rules_rec through sparc_rules_records_device and
SPaRCVecEnv.audit_records): record j gets what k_rules gives an env holding that state
(_validate_rules, SPaRC_Gym.py:941-950), from a context that is never reset and whose env count
has nothing to do with the number of records.

* bits, region map and fit mask against the reference's golden rule_status vectors and, byte for
  byte, against rule_audit() of the context that walks the episodes;
* the table-only kernel (W = 1, every puzzle in the region-code table, bits only) against
  rule_audit(), the oracle (oracle/rules_ref.py) and the generic kernel on the same records;
* record counts around the wave and workgroup sizes; damaged records; refused headers; a queue
  overflow that runs the launch again from the caller's records.
"""
import numpy as np
import pytest

from golden_io import load
from oracle import rules_ref
from rules_io import RULE_POOLS, ref_puzzle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _fit_mask(status):
    m = 0
    for d in status["poly_ylop_area"]["detail"].get("region_details", []):
        if d["ok"]:
            m |= 1 << int(d["region"])
    return m


def _region_bits(refp, s, pitch, words):
    _, rm = rules_ref.RuleAudit(refp, s["path"], s["agent"]).compute_regions()
    out = np.full(64 * words, 255, np.uint8)
    for x in range(rm.shape[0]):
        for y in range(rm.shape[1]):
            if rm[x, y] >= 0:
                out[x * pitch + y] = rm[x, y]
    return out


def _state_points(vis_words, pitch, X, Y):
    v = sum(int(w) << (64 * k) for k, w in enumerate(vis_words))
    return [[x, y] for x in range(X) for y in range(Y) if (v >> (x * pitch + y)) & 1]


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


# ----------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("fit_cap", [None, 1])
@pytest.mark.parametrize("pool", RULE_POOLS)
def test_records_audit_matches_reference(on_gpu, pool, fit_cap):
    """The golden episodes, walked by one context; after the reset and after every step its
    snapshot is audited by a SECOND context of one env on the same puzzles that is never reset.
    fit_cap 1: nearly every exact fit goes through the queue and the host."""
    from sparc_gym_amd import SPaRCVecEnv
    g = load(pool)
    eps = g["episodes"]
    n, T = len(eps), max(len(e["actions"]) for e in eps)
    kw = dict(puzzles=g["records"], traceback=g["traceback"], max_steps=2000, autoreset="none", fit_cap=fit_cap)
    vec = SPaRCVecEnv(n, rules=True, **kw)
    aud = SPaRCVecEnv(1, **kw)
    assert n != aud.num_envs
    refp = [ref_puzzle(p) for p in g["processed"]]
    pitch, words = vec.table.pitch, vec.table.words
    vec.reset(options={"puzzle_index": [e["puzzle_index"] for e in eps]})
    acts = np.full((T, n), 255, np.int64)
    for i, e in enumerate(eps):
        acts[:len(e["actions"]), i] = e["actions"]
    for t in range(-1, T):
        if t >= 0:
            vec.step(torch.from_numpy(acts[t]).cuda())
        before = vec.snapshot()
        got = _np(aud.audit_records(before, region=True, fit=True))
        assert torch.equal(vec.snapshot().records, before.records)          # the walking state is untouched
        want = _np(vec.rule_audit(region=True, fit=True))
        for k in ("bits", "region", "fit"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (pool, t, k)
        only = aud.audit_records(before)["bits"].cpu().numpy()               # bits alone: the hot path
        assert np.array_equal(only, want["bits"]), (pool, t)
        bits, fit = got["bits"].astype(np.uint16), got["fit"].astype(np.uint64)
        for i, e in enumerate(eps):
            if t >= len(e["steps"]):
                continue
            s = e["reset"] if t < 0 else e["steps"][t]
            assert int(bits[i]) == rules_ref.rule_bits(s["rule_status"]), (pool, i, t)
            assert int(fit[i]) == _fit_mask(s["rule_status"]), (pool, i, t)
            want_region = _region_bits(refp[e["puzzle_index"]], s, pitch, words)
            assert np.array_equal(got["region"][i], want_region), (pool, i, t)
    aud.core.sync()
    assert aud.core.has_state is False                                       # never reset


# ----------------------------------------------------------------------------- 2. table-only
N_TAB = 4096


@pytest.fixture(scope="module")
def tab_pool():
    """A W = 1 pool whose every puzzle has a region-code table (7 x 7 lattices): 4,096 envs after a
    40-step random rollout, their snapshot, rule_audit()'s answer, and a one-env auditing
    context."""
    from sparc_gym_amd import SPaRCVecEnv, synthetic
    from sparc_gym_amd.puzzles import pack_table, process_puzzles
    recs = synthetic.make_rule_puzzles(256, seed=8, sizes=((3, 3),), break_prob=0.3)
    recs += synthetic.make_puzzles(256, seed=7, sizes=((3, 3),), full_properties=True)
    proc = process_puzzles(recs)
    table = pack_table(proc)
    kw = dict(processed=proc, table=table, traceback=True, autoreset="next_step", observation="compact")
    vec = SPaRCVecEnv(N_TAB, rules=True, **kw)
    assert vec.table.words == 1
    gid = np.arange(N_TAB, dtype=np.uint64)
    vec.reset(options={"puzzle_index": (gid * 2654435761 % len(proc)).astype(np.int64)})
    vec.rollout(40, None, seed=40, record=False)
    snap = vec.snapshot()
    full = _np(vec.rule_audit(region=True, fit=True))
    aud = SPaRCVecEnv(1, **kw)
    return {"proc": proc, "vec": vec, "aud": aud, "snap": snap, "full": full, "state": vec.state()}


def test_table_only_kernel(on_gpu, tab_pool):
    S = tab_pool
    aud, snap, full = S["aud"], S["snap"], S["full"]
    bits = aud.audit_records(snap)["bits"].cpu().numpy()                     # bits only: k_rules_rec<1, true>
    assert np.array_equal(bits, full["bits"])
    gen = _np(aud.audit_records(snap, region=True))                          # the generic instance
    assert np.array_equal(gen["bits"], bits) and np.array_equal(gen["region"], full["region"])
    fit = _np(aud.audit_records(snap, fit=True))
    assert np.array_equal(fit["bits"], bits) and np.array_equal(fit["fit"], full["fit"])
    host = _np(aud.audit_records(snap.cpu()))                                # a host snapshot
    assert np.array_equal(host["bits"], bits)
    st, refp = S["state"], [dict(p) for p in S["proc"]]
    rng = np.random.default_rng(0)
    for i in rng.choice(N_TAB, size=64, replace=False):
        p = refp[int(st["puzzle"][i])]
        path = _state_points(st["visited"][:, i], aud.table.pitch, p["x_size"], p["y_size"])
        want = rules_ref.rule_bits(rules_ref.audit(p, path, (int(st["x"][i]), int(st["y"][i]))))
        assert int(bits[i].astype(np.uint16)) == want, i
    assert len(np.unique(bits)) > 4
    aud.core.sync()


def test_records_host_form(on_gpu, tab_pool):
    """sparc_rules_records_host: staged records, final answers on the host."""
    S = tab_pool
    aud, full = S["aud"], S["full"]
    aud._load_rules()
    rec = S["snap"].numpy()[:300]
    out = aud.core.rules_records_host(S["snap"].info, rec, region=True, fit=True)
    assert np.array_equal(out["bits"], full["bits"][:300].astype(np.uint16))
    assert np.array_equal(out["region"], full["region"][:300])
    assert np.array_equal(out["fit"], full["fit"][:300].astype(np.uint64))
    only = aud.core.rules_records_host(S["snap"].info, rec)
    assert np.array_equal(only["bits"], out["bits"])


# ----------------------------------------------------------------------------- 3. edges of the grid
@pytest.mark.parametrize("M", [1, 63, 65, 255, 257])
def test_record_counts_around_wave_and_workgroup(on_gpu, tab_pool, M):
    S = tab_pool
    aud, full = S["aud"], S["full"]
    idx = (np.arange(M) * 13 + 5) % N_TAB
    sub = S["snap"].select(idx)
    assert len(sub) == M
    got = _np(aud.audit_records(sub, region=True, fit=True))                 # generic
    for k in ("bits", "region", "fit"):
        assert got[k].shape[0] == M and np.array_equal(got[k], full[k][idx]), k
    guard = torch.full((M + 64,), 0x5A5A, dtype=torch.int16, device="cuda")  # table-only, with a guard past M
    aud.core.rules_records_device(sub.info, sub.records.data_ptr(), M, guard.data_ptr())
    aud.core.rules_finish(guard.data_ptr())
    guard = guard.cpu().numpy()
    assert np.array_equal(guard[:M], full["bits"][idx]) and (guard[M:] == 0x5A5A).all()
    aud.core.sync()


# ----------------------------------------------------------------------------- 4. bad records
def test_bad_records_are_refused_on_the_device(on_gpu, tab_pool):
    from sparc_gym_amd.snapshot import Snapshot
    S = tab_pool
    aud, full, proc = S["aud"], S["full"], S["proc"]
    M = 130
    idx = np.arange(M) * 31 % N_TAB
    clean = S["snap"].select(idx)
    rec = clean.records.clone()
    k_pid, k_zero, k_x = 0, 64, M - 1
    P = len(proc)
    rec[k_pid, 12:16] = torch.tensor(list(int(P).to_bytes(4, "little")), dtype=torch.uint8, device="cuda")
    rec[k_zero] = 0
    q = int(S["state"]["puzzle"][idx[k_x]])
    rec[k_x, 0] = int(proc[q]["x_size"])
    bad = np.zeros(M, bool)
    bad[[k_pid, k_zero, k_x]] = True
    for region, fit in ((True, True), (False, False)):                       # the generic and the table-only kernel
        out = _np(aud.audit_records(Snapshot(rec, clean.info), region=region, fit=fit))
        with pytest.raises(ValueError, match="record"):
            aud.core.sync()
        aud.core.sync()                                                      # the error is reported once
        assert (out["bits"][bad] == 0).all()
        assert np.array_equal(out["bits"][~bad], full["bits"][idx][~bad])
        if region:
            assert (out["fit"][bad] == 0).all() and (out["region"][bad] == 255).all()
            assert np.array_equal(out["fit"][~bad], full["fit"][idx][~bad])
            assert np.array_equal(out["region"][~bad], full["region"][idx][~bad])
    again = _np(aud.audit_records(clean, region=True, fit=True))             # the context is fine afterwards
    for k in ("bits", "region", "fit"):
        assert np.array_equal(again[k], full[k][idx]), k
    aud.core.sync()


# ----------------------------------------------------------------------------- 5. refused on the host
@pytest.mark.parametrize("what", ["max_steps", "table_hash"])
def test_header_mismatch_is_rejected_before_any_launch(on_gpu, tab_pool, what):
    from sparc_gym_amd import SPaRCVecEnv, synthetic
    from sparc_gym_amd.puzzles import pack_table, process_puzzles
    S = tab_pool
    kw = dict(traceback=True, autoreset="next_step", observation="compact")
    if what == "max_steps":
        v = SPaRCVecEnv(2, processed=S["proc"], max_steps=77, **kw)
    else:                          # the same pool with one puzzle exchanged
        proc = list(S["proc"])
        proc[17] = process_puzzles(synthetic.make_puzzles(1, seed=99, sizes=((3, 3),), full_properties=True))[0]
        v = SPaRCVecEnv(2, processed=proc, table=pack_table(proc), **kw)
    s = S["snap"].select(np.arange(10))
    with pytest.raises(ValueError, match=what):
        v.audit_records(s)
    bits = torch.full((10,), 0x5A5A, dtype=torch.int16, device="cuda")
    with pytest.raises(ValueError, match=what):                              # the library's own check
        v.core.rules_records_device(s.info, s.records.data_ptr(), 10, bits.data_ptr())
    v.core.sync()
    assert (bits == 0x5A5A).all()


def test_missing_rules_and_bad_pointers(on_gpu, tab_pool):
    from sparc_gym_amd import SPaRCVecEnv
    from sparc_gym_amd._lib import SparcError
    S = tab_pool
    v = SPaRCVecEnv(2, processed=S["proc"], traceback=True, autoreset="next_step", observation="compact")
    s = S["snap"].select(np.arange(10))
    rb = s.info.record_bytes
    bits = torch.full((10,), 0x5A5A, dtype=torch.int16, device="cuda")
    with pytest.raises(SparcError, match="sparc_load_rules"):                # SPARC_E_STATE: no rules yet
        v.core.rules_records_device(s.info, s.records.data_ptr(), 10, bits.data_ptr())
    with pytest.raises(SparcError, match="sparc_load_rules"):
        v.core.rules_records_host(s.info, s.numpy())
    v._load_rules()
    shifted = torch.empty(10 * rb + 16, dtype=torch.uint8, device="cuda")
    shifted[8:8 + 10 * rb] = s.records.reshape(-1)
    assert shifted.data_ptr() % 16 == 0
    with pytest.raises(ValueError, match="aligned"):
        v.core.rules_records_device(s.info, shifted.data_ptr() + 8, 10, bits.data_ptr())
    with pytest.raises(ValueError, match="records"):
        v.core.rules_records_device(s.info, None, 10, bits.data_ptr())
    with pytest.raises(ValueError, match="bits"):
        v.core.rules_records_device(s.info, s.records.data_ptr(), 10, None)
    for M in (0, 2**31):
        with pytest.raises(ValueError, match="M must"):
            v.core.rules_records_device(s.info, s.records.data_ptr(), M, bits.data_ptr())
    v.core.sync()
    assert (bits == 0x5A5A).all()
    got = v.audit_records(s)["bits"].cpu().numpy()                           # and it audits without a reset
    assert np.array_equal(got, S["full"]["bits"][:10])


# ----------------------------------------------------------------------------- 6. queue overflow
def test_queue_overflow_reruns_from_the_records(on_gpu):
    """The pool of test_exact_fit_queue_overflow_rerun (two-walled 15 x 15 puzzles: two exact-fit
    searches per audit, no region-code table), fit_cap = 1 and the host's answers not kept: 70,000
    records queue 140,000 searches, more than the queue's first 65,536 entries, so the finish grows
    the queue and runs the launch again from the same records.  The answers equal the default
    cap's (every search on the GPU)."""
    from sparc_gym_amd import SPaRCVecEnv, synthetic
    from sparc_gym_amd.puzzles import pack_table, process_puzzles
    from test_gpu_rules_limits import _two_walls
    recs = [r for r in map(_two_walls, synthetic.make_puzzles(200, seed=41, sizes=((7, 7),), full_properties=False,
                                                                n_solutions=1)) if r is not None]
    assert len(recs) > 50
    proc = process_puzzles(recs)
    table = pack_table(proc)
    kw = dict(processed=proc, table=table, traceback=True, autoreset="next_step", observation="compact",
              max_steps=40)
    n, M = 384, 70000
    walk = SPaRCVecEnv(n, **kw)
    walk.reset(options={"puzzle_index": np.arange(n) % len(proc)})
    walk.rollout(7, None, seed=3, record=False)
    snap = walk.snapshot().select(np.arange(M) % n)                          # a few hundred states, repeated
    outs = []
    for cap in (1, None):
        v = SPaRCVecEnv(1, fit_cap=cap, **kw)
        v._load_rules()
        v.core.set_variant(v.core.VARIANT_HOST_FITS, 1)
        outs.append((_np(v.audit_records(snap, region=True, fit=True)), v))
    (a, va), (b, vb) = outs
    for k in ("bits", "region", "fit"):
        assert np.array_equal(a[k], b[k]), k
    assert not (a["bits"].astype(np.uint16) & (1 << 9)).any()
    assert va.core.rules_queue_stats()["capacity"] > 65536                   # the queue grew: the call ran again
    assert va.core.rules_queue_stats()["reruns"] >= 1 and vb.core.rules_queue_stats()["reruns"] == 0
    assert np.array_equal(a["bits"][:n], a["bits"][n:2 * n])
    va.core.sync()
