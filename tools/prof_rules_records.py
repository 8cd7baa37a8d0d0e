#!/usr/bin/env python3
"""Device time of sparc_rules_records_device (bits only) against the path it replaces.

Shapes: M = 65,536 and 262,144 records of the c3r bench pool (7x7, one word, traceback, every
puzzle in the region-code table: the table-only kernel) and of the mixed 5x5-11x11 pool (two
words, traceback: the generic kernel).  The records are the states of M envs after 64 random
steps.  The replaced path is what a search had to do before: sparc_restore_device of the M
records into a context of M envs, then sparc_rules_device; two launches timed as one unit.  Both
entry points exist unchanged on the parent commit and are the yardstick.  Each path is timed with
device events on its context's stream (both contexts share it), after a warm-up, in rounds that
alternate the two on the same box; the median of `--calls` rounds is reported, and the medians
of the four quarters of the rounds, whose spread for the replaced path is the margin within which
the two count as equal.  The replaced path keeps its per-env exact-fit memo in HBM between
rounds, and every round audits the same states: on the two-word pool its searches are memo hits
after the first round, which the records audit (no memo) repeats every time.  A third figure,
reported beside the two, is the replaced path with an empty memo, as its first audit of a new
frontier meets it: `--empty-rounds` more rounds in which sparc_load_rules (untimed) zeroes the memo
before the replaced path is timed (`replaced_empty_memo`).
The bits of the two paths are compared at the timed sizes after their sparc_rules_finish.

Every shape runs in a child process of its own under `timeout`; the first one that fails or
overruns ends the run."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOLS = {"c3r": "c3r (7x7, W=1, traceback, table-only)", "c4c": "mixed 5x5-11x11 (W=2, traceback, generic)"}
WARM = 20

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200, help="timed rounds (each path once per round)")
ap.add_argument("--empty-rounds", type=int, default=10, help="rounds of the replaced path on an empty memo")
ap.add_argument("--records", type=int, nargs="+", default=[65536, 262144])
ap.add_argument("--puzzles", type=int, default=1024)
ap.add_argument("--limit", type=int, default=240, help="seconds allowed to one shape")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rules_records", "prof_rules_records.json"))
ap.add_argument("--worker", nargs=2, metavar=("POOL", "M"), help=argparse.SUPPRESS)
a = ap.parse_args()
if a.calls < 200:
    sys.exit("--calls must be at least 200 (the medians are quoted in DESIGN.md)")


def worker(cfg, M):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "sparc-gym_amd"))
    import numpy as np
    import torch

    import bench
    from sparc_gym_amd import SPaRCVecEnv, synthetic
    from sparc_gym_amd.puzzles import pack_rules, pack_table, process_puzzles

    sizes, full, tb, _ = bench.CONFIGS[cfg]
    proc = process_puzzles(synthetic.make_puzzles(a.puzzles, seed=0, sizes=sizes, full_properties=full))
    table = pack_table(proc)
    kw = dict(processed=proc, table=table, traceback=tb, observation="compact")
    v = SPaRCVecEnv(M, rules=True, **kw)                     # the states, and the replaced path's M-env context
    v.reset(options={"puzzle_index": np.arange(M) % len(proc)})
    v.rollout(64, None, seed=1, record=False)
    aud = SPaRCVecEnv(1, **kw)                               # the records audit: one env, never reset
    aud._stream()
    aud._load_rules()
    W, dev = table.words, v.device
    info = v.core.snapshot_info()
    rb = info.record_bytes
    state = 16 + 8 * W + (16 * W if tb else 0)              # bytes of one env in the SoA arrays
    recs = v.snapshot().records
    bits_a = torch.empty(M, dtype=torch.int16, device=dev)
    bits_b = torch.empty(M, dtype=torch.int16, device=dev)

    def records():
        aud.core.rules_records_device(info, recs.data_ptr(), M, bits_a.data_ptr())

    def replaced():
        v.core.restore_device(info, recs.data_ptr(), M)
        v.core.rules_device(bits_b.data_ptr())

    read = 16 * ((4 + 2 * W + 3) // 4)                      # the pieces of a record the records audit reads
    nbytes = {"records": M * (read + 2), "replaced": M * (rb + state) + M * (16 + 8 * W + 2 + 2 * 48)}
    ops = {"records": records, "replaced": replaced}
    times = {k: [] for k in ops}
    stream = torch.cuda.current_stream(dev)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        f()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for r in range(WARM + a.calls):
        for name, f in ops.items():
            t = timed(f)
            if r >= WARM:
                times[name].append(t)
    rules = pack_rules(proc, table)
    empty = []
    for r in range(a.empty_rounds):
        v.core.load_rules(rules)                            # zeroes the per-env memo (untimed)
        v.core.sync()
        empty.append(timed(replaced))
    # final bits of both paths (each context finishes its own last call), then the comparison
    replaced()
    v.core.rules_finish(bits_b.data_ptr())
    records()
    aud.core.rules_finish(bits_a.data_ptr())
    v.core.sync()
    aud.core.sync()
    equal = bool(torch.equal(bits_a, bits_b))
    med = {k: float(np.median(t)) for k, t in times.items()}
    quarters = {k: [float(np.median(c)) for c in np.array_split(np.asarray(t), 4)] for k, t in times.items()}
    spread = max(quarters["replaced"]) - min(quarters["replaced"])
    row = {"pool": POOLS[cfg], "records": M, "words": W, "traceback": bool(tb), "record_bytes": rb,
           "bytes_read_per_record": read, "rounds": a.calls, "bits_equal": equal,
           "distinct_bit_words": int(len(torch.unique(bits_a))),
           "records_vs_replaced": round(med["records"] / med["replaced"], 3),
           "replaced_empty_memo": {"median_us": round(float(np.median(empty)), 2), "rounds": len(empty)},
           "records_vs_replaced_empty_memo": round(med["records"] / float(np.median(empty)), 3),
           "replaced_quarter_median_spread_us": round(spread, 2),
           "records_slower_than_spread": bool(med["records"] > med["replaced"] + spread)}
    for k in ops:
        t = times[k]
        row[k] = {"median_us": round(med[k], 2), "p10_us": round(float(np.percentile(t, 10)), 2),
                  "p90_us": round(float(np.percentile(t, 90)), 2),
                  "quarter_medians_us": [round(q, 2) for q in quarters[k]], "bytes_moved": nbytes[k],
                  "launches": 1 if k == "records" else 2}
    row["device"] = torch.cuda.get_device_name(0)
    v.close()
    aud.close()
    print("ROW " + json.dumps(row), flush=True)


if a.worker:
    worker(a.worker[0], int(a.worker[1]))
    sys.exit(0)

rows = []
for cfg in POOLS:
    for M in a.records:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", cfg, str(M),
               "--calls", str(a.calls), "--puzzles", str(a.puzzles), "--empty-rounds", str(a.empty_rounds)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")), None)
        if p.returncode != 0 or line is None:
            sys.exit(f"{POOLS[cfg]} M={M}: the GPU step ended with status {p.returncode}; nothing more is run")
        row = json.loads(line[4:])
        rows.append(row)
        print(f"{row['pool']:42s} M={M:7d} records {row['records']['median_us']:9.2f} us  replaced "
              f"{row['replaced']['median_us']:9.2f} us  ratio {row['records_vs_replaced']:.3f}  empty memo "
              f"{row['replaced_empty_memo']['median_us']:9.2f} us  ratio {row['records_vs_replaced_empty_memo']:.3f}  "
              f"spread of replaced {row['replaced_quarter_median_spread_us']:.2f} us  equal {row['bits_equal']}",
              flush=True)

device = rows[0].pop("device")
for r in rows[1:]:
    r.pop("device")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump({"device": device, "timing": "device events around one path, median; the two paths alternate in rounds "
               f"after {WARM} warm-up rounds", "bytes": "computed from the shapes, not measured (the replaced path: "
               "restore reads the record and writes the state, the audit reads pos, pid and the board, reads and "
               "writes the 48-B memo and writes the bits)", "rows": rows}, f, indent=1)
print("wrote", a.out)
bad = [r for r in rows if not r["bits_equal"]]
if bad:
    sys.exit("the two paths' bits differ at: " + ", ".join(f"{r['pool']} M={r['records']}" for r in bad))
