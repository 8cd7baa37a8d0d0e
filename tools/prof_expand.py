#!/usr/bin/env python3
"""Device time of sparc_expand_device against the composed path it replaces.

Shapes: M = 65,536 and 262,144 parent records of the c3 pool (7x7, one word, traceback) and of
the mixed 5x5-11x11 pool (two words, traceback).  The parents are the states of M envs after 64
random steps.  The composed path is what a search had to do before: sparc_restore_device into a
context of 4 * M envs with src = j // 4, sparc_step_device with action j % 4, and
sparc_snapshot_device, three launches timed as one unit.  It exists unchanged on the parent
commit and is the yardstick.  Each path is timed with device events on the context's stream,
after a warm-up, in rounds that alternate the two on the same box; the median of `--calls` rounds
is reported, with the bytes each path moves (computed from the shapes, not measured) and the
fraction of the 8 TB/s HBM peak that expand's bytes over its time come to.  The children, codes
and flags of expand are compared once per shape with the composed path run on a 65,536-env
context, 16,384 parents at a time (`results_equal`), and with the timed composed path itself
(`results_equal_at_4M_envs`, reported only).

Every shape runs in a child process of its own under `timeout`; the first one that fails or
overruns ends the run."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOLS = {"c3": "c3 (7x7, W=1, traceback)", "c4c": "mixed 5x5-11x11 (W=2, traceback)"}
HBM_PEAK = 8.0e12   # B/s, the HBM3E specification of the MI355X
WARM = 20

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200, help="timed rounds (each path once per round)")
ap.add_argument("--parents", type=int, nargs="+", default=[65536, 262144])
ap.add_argument("--puzzles", type=int, default=1024)
ap.add_argument("--limit", type=int, default=240, help="seconds allowed to one shape")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "expand", "prof_expand.json"))
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
    from sparc_gym_amd.puzzles import pack_table, process_puzzles

    sizes, full, tb, _ = bench.CONFIGS[cfg]
    proc = process_puzzles(synthetic.make_puzzles(a.puzzles, seed=0, sizes=sizes, full_properties=full))
    table = pack_table(proc)
    n = 4 * M
    v = SPaRCVecEnv(n, processed=proc, table=table, traceback=tb, observation="compact")
    v.reset(options={"puzzle_index": np.arange(n) % len(proc)})
    v.rollout(64, None, seed=1, record=False)
    core, W, dev = v.core, table.words, v.device
    info = core.snapshot_info()
    rb = info.record_bytes
    state = 16 + 8 * W + (16 * W if tb else 0)              # bytes of one env in the SoA arrays
    parents = v.snapshot(envs=torch.arange(M, dtype=torch.int32, device=dev)).records
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)   # noqa: E731
    kids, code, flags, pflags = u8(n, rb), torch.empty(n, dtype=torch.int8, device=dev), u8(n), u8(M)
    kids2, code2, flags2, rflags = u8(n, rb), torch.empty(n, dtype=torch.int8, device=dev), u8(n), u8(n)
    src = (torch.arange(n, dtype=torch.int32, device=dev) // 4).contiguous()
    acts = (torch.arange(n, device=dev) % 4).to(torch.uint8)

    def expand():
        core.expand_device(info, parents.data_ptr(), M, kids.data_ptr(), code.data_ptr(), flags.data_ptr(),
                           pflags.data_ptr())

    def composed():
        core.restore_device(info, parents.data_ptr(), M, src.data_ptr(), None, rflags.data_ptr())
        core.step_device(acts.data_ptr(), code2.data_ptr(), flags2.data_ptr())
        core.snapshot_device(None, n, kids2.data_ptr())

    nbytes = {"expand": M * (rb + 4 * rb + 4 + 4 + 1),
              "composed": M * rb + n * (4 + state + 1) + n * (state + 1 + state + 2) + n * (state + rb)}
    ops = {"expand": expand, "composed": composed}
    times = {k: [] for k in ops}
    stream = torch.cuda.current_stream(dev)
    for r in range(WARM + a.calls):
        for name, f in ops.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            f()
            e1.record(stream)
            e1.synchronize()
            if r >= WARM:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    core.sync()
    equal = bool(torch.equal(kids, kids2) and torch.equal(code, code2) and torch.equal(flags, flags2)
                 and torch.equal(pflags, rflags[::4]))
    # the same comparison with the composed path on a context of 65,536 envs, 16,384 parents at a
    # time (see profiles/expand/README.md: at W = 1 with traceback the one-step kernel was seen to
    # return direction stacks that vary from run to run for envs past the first 65,536)
    C = 16384
    small = SPaRCVecEnv(4 * C, processed=proc, table=table, traceback=tb, observation="compact")
    small._stream()                                         # the stream of the comparisons below
    chunks_equal = M % C == 0
    for lo in range(0, M, C):
        small.core.restore_device(info, parents[lo:lo + C].data_ptr(), C, src.data_ptr(), None, rflags.data_ptr())
        small.core.step_device(acts.data_ptr(), code2.data_ptr(), flags2.data_ptr())
        small.core.snapshot_device(None, 4 * C, kids2.data_ptr())
        s4 = slice(4 * lo, 4 * (lo + C))
        chunks_equal &= bool(torch.equal(kids[s4], kids2[:4 * C]) and torch.equal(code[s4], code2[:4 * C])
                             and torch.equal(flags[s4], flags2[:4 * C])
                             and torch.equal(pflags[lo:lo + C], rflags[:4 * C:4]))
    small.core.sync()
    small.close()
    med = {k: float(np.median(t)) for k, t in times.items()}
    row = {"pool": POOLS[cfg], "parents": M, "children": n, "words": W, "traceback": bool(tb), "record_bytes": rb,
           "state_bytes_per_env": state, "rounds": a.calls, "results_equal": chunks_equal,
           "results_equal_at_4M_envs": equal,
           "expand_vs_composed": round(med["expand"] / med["composed"], 3),
           "expand_fraction_of_hbm_peak": round(nbytes["expand"] / (med["expand"] * 1e-6) / HBM_PEAK, 3)}
    for k in ops:
        t = times[k]
        row[k] = {"median_us": round(med[k], 2), "p10_us": round(float(np.percentile(t, 10)), 2),
                  "p90_us": round(float(np.percentile(t, 90)), 2), "bytes_moved": nbytes[k],
                  "GB_per_s": round(nbytes[k] / med[k] / 1e3, 1), "launches": 1 if k == "expand" else 3}
    row["device"] = torch.cuda.get_device_name(0)
    v.close()
    print("ROW " + json.dumps(row), flush=True)


if a.worker:
    worker(a.worker[0], int(a.worker[1]))
    sys.exit(0)

rows = []
for cfg in POOLS:
    for M in a.parents:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", cfg, str(M),
               "--calls", str(a.calls), "--puzzles", str(a.puzzles)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")), None)
        if p.returncode != 0 or line is None:
            sys.exit(f"{POOLS[cfg]} M={M}: the GPU step ended with status {p.returncode}; nothing more is run")
        row = json.loads(line[4:])
        rows.append(row)
        print(f"{row['pool']:34s} M={M:7d} expand {row['expand']['median_us']:8.2f} us  composed "
              f"{row['composed']['median_us']:8.2f} us  ratio {row['expand_vs_composed']:.3f}  "
              f"{row['expand']['GB_per_s']:7.1f} GB/s = {row['expand_fraction_of_hbm_peak']:.3f} of peak  "
              f"equal {row['results_equal']} (composed at 4M envs: {row['results_equal_at_4M_envs']})", flush=True)

device = rows[0].pop("device")
for r in rows[1:]:
    r.pop("device")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump({"device": device, "timing": "device events around one path, median; the two paths alternate in rounds "
               f"after {WARM} warm-up rounds", "hbm_peak_B_per_s": HBM_PEAK,
               "bytes": "computed from the shapes, not measured", "rows": rows}, f, indent=1)
print("wrote", a.out)
bad = [r for r in rows if not r["results_equal"] or r["expand_vs_composed"] >= 1.0]
if bad:
    sys.exit("expand is not faster than the composed path, or differs from it, at: " +
             ", ".join(f"{r['pool']} M={r['parents']}" for r in bad))
