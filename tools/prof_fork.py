#!/usr/bin/env python3
"""Device time of snapshot / restore / fork against sparc_reset_device at the same N.

Shapes: 65,536 and 262,144 envs of the c3 pool (7x7, one word, traceback) and of the mixed
5x5-11x11 pool (two words, traceback).  Every call is timed on its own with device events on the
context's stream, after a warm-up, in rounds that alternate the calls with sparc_reset_device on
the same context; the median of `--calls` rounds is reported.  The yardstick is the reset, which
writes the same state arrays once; a restore also reads one record per env, and a fork moves the
state twice (k_snapshot into the context's scratch, then k_restore).  The JSON also holds the
bytes each call moves, computed from the shapes."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "sparc-gym_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from sparc_gym_amd import SPaRCVecEnv, synthetic  # noqa: E402
from sparc_gym_amd.puzzles import pack_table, process_puzzles  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200, help="timed rounds (each call once per round)")
ap.add_argument("--envs", type=int, nargs="+", default=[65536, 262144])
ap.add_argument("--puzzles", type=int, default=1024)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fork", "prof_fork.json"))
a = ap.parse_args()
if a.calls < 200:
    sys.exit("--calls must be at least 200 (the medians are quoted in DESIGN.md)")

POOLS = {"c3 (7x7, W=1, traceback)": "c3", "mixed 5x5-11x11 (W=2, traceback)": "c4c"}
rows = []
for label, cfg in POOLS.items():
    sizes, full, tb, _ = bench.CONFIGS[cfg]
    proc = process_puzzles(synthetic.make_puzzles(a.puzzles, seed=0, sizes=sizes, full_properties=full))
    table = pack_table(proc)
    for n in a.envs:
        v = SPaRCVecEnv(n, processed=proc, table=table, traceback=tb, observation="compact")
        v.reset(options={"puzzle_index": np.arange(n) % len(proc)})
        v.rollout(64, None, seed=1, record=False)
        core, W = v.core, table.words
        info = core.snapshot_info()
        rb = info.record_bytes
        state = 16 + 8 * W + (16 * W if tb else 0)          # bytes of one env in the SoA arrays
        dev = v.device
        g = torch.Generator(device="cpu").manual_seed(0)
        pidx = (torch.arange(n, dtype=torch.int32) % len(proc)).to(dev)
        rnd = torch.randint(0, n, (n,), generator=g, dtype=torch.int32).to(dev)
        perm = torch.randperm(n, generator=g).to(torch.int32).to(dev)
        one = torch.full((n,), 7, dtype=torch.int32, device=dev)
        flags = torch.zeros(n, dtype=torch.uint8, device=dev)
        rec0 = torch.empty((n, rb), dtype=torch.uint8, device=dev)
        rec1 = torch.empty_like(rec0)
        core.snapshot_device(None, n, rec0.data_ptr())
        ops = {
            "reset": (lambda: core.reset_device(pidx.data_ptr(), None, flags.data_ptr()), n * (state + 4 + 1)),
            "snapshot": (lambda: core.snapshot_device(None, n, rec1.data_ptr()), n * (state + rb)),
            "restore_identity": (lambda: core.restore_device(info, rec0.data_ptr(), n, None, None, flags.data_ptr()),
                                 n * (rb + state + 1)),
            "restore_random_src": (lambda: core.restore_device(info, rec0.data_ptr(), n, rnd.data_ptr(), None,
                                                               flags.data_ptr()), n * (rb + 4 + state + 1)),
            "fork_permutation": (lambda: core.fork_device(perm.data_ptr(), None, flags.data_ptr()),
                                 n * (2 * state + 2 * rb + 4 + 1)),
            "fork_all_from_one": (lambda: core.fork_device(one.data_ptr(), None, flags.data_ptr()),
                                  n * (2 * state + 2 * rb + 4 + 1)),
        }
        # a round: every call once, a reset before each, the state brought back in between
        order = ["reset", "snapshot", "reset", "restore_identity", "fork_permutation", "reset", "restore_random_src",
                 "fork_all_from_one"]
        times = {k: [] for k in ops}
        stream = torch.cuda.current_stream(dev)
        for r in range(20 + a.calls):
            for name in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                ops[name][0]()
                e1.record(stream)
                e1.synchronize()
                if r >= 20:
                    times[name].append(e0.elapsed_time(e1) * 1e3)
        core.sync()
        med = {k: float(np.median(t)) for k, t in times.items()}
        for k in ops:
            rows.append({"pool": label, "envs": n, "words": W, "traceback": bool(tb), "record_bytes": rb,
                         "state_bytes_per_env": state, "call": k, "calls": len(times[k]), "median_us": round(med[k], 2),
                         "p10_us": round(float(np.percentile(times[k], 10)), 2),
                         "p90_us": round(float(np.percentile(times[k], 90)), 2),
                         "bytes_moved": ops[k][1], "GB_per_s": round(ops[k][1] / med[k] / 1e3, 1),
                         "vs_reset": round(med[k] / med["reset"], 2)})
            print(f"{label:34s} N={n:7d} {k:20s} {med[k]:8.2f} us  x{med[k] / med['reset']:.2f} of reset  "
                  f"{ops[k][1] / med[k] / 1e3:7.1f} GB/s", flush=True)
        v.close()

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump({"device": torch.cuda.get_device_name(0), "timing": "device events around one call, median",
               "launches_per_call": {"reset": 1, "snapshot": 1, "restore": 1, "fork": 2}, "rows": rows}, f, indent=1)
print("wrote", a.out)
