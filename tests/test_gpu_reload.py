"""A table load that fails leaves the context as it was; a valid reload replaces it as a whole."""
import numpy as np
import pytest

from oracle import COracle
from sparc_gym_amd import synthetic
from sparc_gym_amd._lib import SparcError
from sparc_gym_amd.puzzles import pack_rules, pack_table, process_puzzles
from test_gpu_parity import oracle_pool_from_processed

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def test_failed_load_keeps_the_tables_and_a_reload_swaps_them(on_gpu):
    from sparc_gym_amd import SPaRCVecEnv
    n, T = 256, 32
    recs = synthetic.make_rule_puzzles(8, seed=41, sizes=((3, 3),), break_prob=0.3)
    recs += synthetic.make_puzzles(8, seed=42, sizes=((3, 3),), full_properties=True)
    proc_a = process_puzzles(recs)
    table_a = pack_table(proc_a)
    rules_a = pack_rules(proc_a, table_a)
    vec = SPaRCVecEnv(n, processed=proc_a, table=table_a, traceback=True, autoreset="next_step",
                      observation="compact", rules=True, max_steps=12)
    core = vec.core
    pids = (np.arange(n) * 5) % len(proc_a)
    acts = torch.randint(0, 4, (T, n), dtype=torch.uint8, device="cuda")

    def run():
        vec.reset(options={"puzzle_index": pids})
        out = vec.rollout(T, acts, rules=True)
        return {k: v.cpu().numpy() for k, v in out.items()}

    first = run()
    assert len(np.unique(first["rule_bits"])) > 4
    # a puzzle table with one child index out of range, a rule table with one bad instance
    q = int(np.flatnonzero((table_a.info[:, 1] >> 16) & 2)[0])
    base, cnt = int(table_a.info[q, 2]), int(table_a.info[q, 3])
    bad_t = pack_table(proc_a)
    bad_t.trie[base, 0] = (int(bad_t.trie[base, 0]) & ~0xFFFF) | cnt
    with pytest.raises(ValueError, match="^trie child out of range$"):
        core.load_table(bad_t)
    bad_r = pack_rules(proc_a, table_a)
    assert len(bad_r.inst) > 0
    bad_r.inst[0] = (int(bad_r.inst[0]) & 0x7FF) | (len(bad_r.shape_area) << 11)
    with pytest.raises(ValueError, match="^bad instance$"):
        core.load_rules(bad_r)
    second = run()
    for k in ("reward_code", "flags", "rule_bits"):
        assert np.array_equal(first[k], second[k]), k
    # a valid pool B replaces A as a whole: no state, no rules until both are set again
    proc_b = process_puzzles(synthetic.make_puzzles(16, seed=43, sizes=((3, 3), (2, 2))))
    table_b = pack_table(proc_b, pitch=table_a.pitch, words=1)
    core.load_table(table_b)
    rew = torch.empty((T, n), dtype=torch.int8, device="cuda")
    flags = torch.empty((T, n), dtype=torch.uint8, device="cuda")
    bits = torch.empty(n, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(SparcError, match="sparc error -3: sparc_reset has not been called"):
        core.step_device(acts.data_ptr(), rew.data_ptr(), flags.data_ptr())
    pids_b = (np.arange(n) * 3) % len(proc_b)
    core.reset_host(pids_b)
    with pytest.raises(SparcError, match="sparc error -3: sparc_load_rules has not been called"):
        core.rules_device(bits.data_ptr())
    core.load_rules(pack_rules(proc_b, table_b))
    core.rules_device(bits.data_ptr())
    core.rules_finish(bits.data_ptr())
    core.reset_host(pids_b)
    core.rollout_device(T, acts.data_ptr(), rew.data_ptr(), flags.data_ptr())
    core.sync()
    o = COracle(oracle_pool_from_processed(proc_b), n, True, 12, autoreset=1)
    o.reset(pids_b)
    r, f = o.rollout(T, acts.cpu().numpy())
    assert np.array_equal(rew.cpu().numpy(), r)
    assert np.array_equal(flags.cpu().numpy(), f)
