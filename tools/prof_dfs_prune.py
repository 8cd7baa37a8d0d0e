#!/usr/bin/env python3
"""Device time, nodes and time to the same answer of the pruned depth-first search
(sparc_dfs_pruned_device, prune 1 and 3) against the unpruned one (prune 0).

Workload: that of tools/prof_dfs.py.  The c3 bench pool (7x7, one word, traceback, max_steps 2000,
1,024 puzzles); the roots are the depth-`--depth` forward frontier of every puzzle's reset state
(search.expand_frontier with the pops dropped, live nodes only), repeated to fill 65,536 records.

  launch    one launch on the 65,536 roots from a fresh state word, for each prune mode and each
            budget: the launch time (device events around it), the nodes it entered, the target
            leaves it audited and the nodes per second.  State, counters and first records are
            cleared outside the timed region.
  complete  the figure a user cares about: launches of `--complete-budget` nodes from a fresh state
            word until every walk is done, the cursor fed back, one synchronisation per launch to
            read the done flags (as search.solve_dfs does it): wall time and launches.  The five
            target counters summed over the roots, and a checksum of the first records, are kept per
            mode; the parent process refuses to write a result unless all modes agree on them.

The prune = 0 rows go through the same entry point (sparc_dfs_pruned_device with prune = 0: the
unpruned kernel behind the state-word check); the yardstick on the parent commit's build is
tools/prof_dfs.py run there.  Each path is timed after `WARM` warm-up runs; the median of `--calls`
runs is reported with the 10th and 90th percentiles.  Every path runs in a child process of its own
under `timeout`; the first one that fails or overruns ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 3

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=15, help="timed runs of each path")
ap.add_argument("--roots", type=int, default=65536)
ap.add_argument("--depth", type=int, default=4, help="forward levels from the reset states to the roots")
ap.add_argument("--budgets", type=int, nargs="+", default=[256, 4096])
ap.add_argument("--complete-budget", type=int, default=4096)
ap.add_argument("--modes", type=int, nargs="+", default=[0, 1, 3])
ap.add_argument("--puzzles", type=int, default=1024)
ap.add_argument("--limit", type=int, default=240, help="seconds allowed to one path")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dfs_prune", "prof_dfs_prune.json"))
ap.add_argument("--worker", nargs=3, metavar=("PATH", "PRUNE", "BUDGET"), help=argparse.SUPPRESS)
a = ap.parse_args()


def worker(path, prune, budget):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "sparc-gym_amd"))
    import numpy as np
    import torch

    import bench
    from sparc_gym_amd import SPaRCVecEnv, _lib, search, synthetic
    from sparc_gym_amd.puzzles import pack_table, process_puzzles

    sizes, full, tb, _ = bench.CONFIGS["c3"]
    proc = process_puzzles(synthetic.make_puzzles(a.puzzles, seed=0, sizes=sizes, full_properties=full))
    v = SPaRCVecEnv(len(proc), processed=proc, table=pack_table(proc), traceback=tb, max_steps=2000,
                    observation="compact", autoreset="none")
    v._load_rules()
    v.reset(options={"puzzle_index": np.arange(len(proc))})

    frontier = v.snapshot()
    for _ in range(a.depth):
        out = search.expand_frontier(v, frontier)
        ch, par = out["children"], out["parent"]
        keep = (ch.fields()["path_len"] > frontier.fields()["path_len"][par]).nonzero().squeeze(1)
        ch, flags = ch.select(keep), out["flags"][keep]
        frontier = ch.select(((flags & 3) == 0).nonzero().squeeze(1))
    distinct = len(frontier)
    roots = frontier.select(torch.arange(a.roots, device=v.device) % distinct)
    M, info, rb, dev = a.roots, roots.info, roots.info.record_bytes, v.device
    row = {"path": path, "prune": prune, "budget": budget, "roots": M, "distinct_roots": distinct,
           "root_depth": a.depth, "runs": a.calls}
    stream = torch.cuda.current_stream(dev)
    v._stream()
    state = torch.zeros(M, dtype=torch.int32, device=dev)
    counts = torch.zeros((M, _lib.DFS_COUNTERS), dtype=torch.int64, device=dev)
    first = torch.zeros((M, rb), dtype=torch.uint8, device=dev)
    status = torch.zeros(M, dtype=torch.uint8, device=dev)
    cursor = torch.empty((M, rb), dtype=torch.uint8, device=dev)

    def launch(src):
        v.core.dfs_device(info, src.data_ptr(), M, budget, state.data_ptr(), status.data_ptr(), counts.data_ptr(),
                          cursor.data_ptr(), first.data_ptr(), prune=prune)

    times, launches = [], 0
    for r in range(WARM + a.calls):
        state.zero_(), counts.zero_(), first.zero_()
        if path == "launch":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch(roots.records)
            e1.record(stream)
            e1.synchronize()
            t = e0.elapsed_time(e1) * 1e3
        else:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            launch(roots.records)
            launches = 1
            while not bool(((state & _lib.DFS_STATE_DONE) != 0).all()):
                launch(cursor)                                        # the cursor written over itself
                launches += 1
            torch.cuda.synchronize(dev)
            t = (time.perf_counter() - t0) * 1e6
        if r >= WARM:
            times.append(t)
    v.core.sync()
    c = counts.sum(0).cpu().tolist()
    st = torch.bincount(status.to(torch.int64), minlength=5).cpu().tolist()
    row.update(nodes=c[_lib.DFS_NODES], counters=dict(zip(_lib.DFS_COUNTER_NAMES, c)), status_0_to_4=st)
    if path == "complete":
        weights = torch.arange(1, rb + 1, dtype=torch.int64, device=dev)
        row.update(launches=launches, first_checksum=int((first.to(torch.int64) * weights).sum()),
                   per_root_targets_checksum=int((counts[:, 1:5] * torch.arange(1, M + 1, device=dev)[:, None]).sum()))
    med = float(np.median(times))
    row.update(median_us=round(med, 2), p10_us=round(float(np.percentile(times, 10)), 2),
               p90_us=round(float(np.percentile(times, 90)), 2),
               nodes_per_second=round(row["nodes"] / (med * 1e-6), 1),
               device=torch.cuda.get_device_name(0))
    v.close()
    print("ROW " + json.dumps(row), flush=True)


if a.worker:
    worker(a.worker[0], int(a.worker[1]), int(a.worker[2]))
    sys.exit(0)

rows = []
jobs = [("launch", m, b) for b in a.budgets for m in a.modes] + [("complete", m, a.complete_budget) for m in a.modes]
for path, mode, budget in jobs:
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", path, str(mode),
           str(budget), "--calls", str(a.calls), "--roots", str(a.roots), "--depth", str(a.depth),
           "--puzzles", str(a.puzzles)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    line = next((ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")), None)
    if p.returncode != 0 or line is None:
        sys.exit(f"{path} prune {mode} budget {budget}: the GPU step ended with status {p.returncode}; "
                 "nothing more is run")
    row = json.loads(line[4:])
    rows.append(row)
    print(f"{path:8s} prune {mode} budget {budget:5d}: {row['median_us']:12.2f} us  nodes {row['nodes']:12d}  "
          f"targets {row['counters']['targets']:9d}  {row['nodes_per_second']:.4g} nodes/s"
          + (f"  launches {row['launches']}" if path == "complete" else ""), flush=True)

# time to the same answer: every mode must report the same target counters and first records
done = [r for r in rows if r["path"] == "complete"]
keys = ("targets", "satisfied", "listed", "both", "undecided")
for r in done[1:]:
    same = all(r["counters"][k] == done[0]["counters"][k] for k in keys) and all(
        r[k] == done[0][k] for k in ("first_checksum", "per_root_targets_checksum"))
    if not same or r["status_0_to_4"][1] != r["roots"]:
        sys.exit(f"prune {r['prune']} does not give the answer of prune {done[0]['prune']}: nothing written")
device = rows[0].pop("device")
for r in rows[1:]:
    r.pop("device")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump({"device": device, "timing": f"median of {a.calls} runs after {WARM} warm-up runs; launch: device events "
               "around one launch; complete: wall time from the first launch until every walk is done, one "
               "synchronisation per launch", "answers_equal": True, "rows": rows}, f, indent=1)
print("wrote", a.out)
