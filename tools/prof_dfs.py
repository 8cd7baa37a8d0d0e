#!/usr/bin/env python3
"""Device time and node rate of sparc_dfs_device against the level loop it replaces.

Workload: the c3 bench pool (7x7, one word, traceback, max_steps 2000, 1,024 puzzles).  The roots
are the depth-`--depth` forward frontier of every puzzle's reset state (search.expand_frontier with
the pops dropped, live nodes only), repeated to fill 65,536 records.

  dfs      one sparc_dfs_device launch on the 65,536 roots from a fresh state word, at budgets 256
           and 4,096: the launch time, the nodes it entered and the nodes per second.  State,
           counters and first records are cleared outside the timed region.
  levels   what the parent commit offers for the same work, the level loop of search.solve_by_rules
           on the same roots: per level one expand launch, the compaction in torch (the pops
           dropped, the live children gathered) and audit_records of the children on the target,
           for `--levels` levels or until a level would pass 2^22 nodes.  Its time is the wall time
           of the whole loop with one synchronisation at the end of each level (the compaction
           needs the level's size on the host anyway); its nodes are the children it kept.

The two paths do not enter the same nodes (depth-first under a budget against breadth-first under a
depth), so the figure to compare is nodes per second on the same roots.  Each path is timed after
`WARM` warm-up runs; the median of `--calls` runs is reported with the 10th and 90th percentiles.
Every path runs in a child process of its own under `timeout`; the first one that fails or overruns
ends the run."""
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
ap.add_argument("--levels", type=int, default=6, help="levels of the level loop")
ap.add_argument("--budgets", type=int, nargs="+", default=[256, 4096])
ap.add_argument("--puzzles", type=int, default=1024)
ap.add_argument("--limit", type=int, default=240, help="seconds allowed to one path")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dfs", "prof_dfs.json"))
ap.add_argument("--worker", nargs=2, metavar=("PATH", "ARG"), help=argparse.SUPPRESS)
a = ap.parse_args()


def worker(path, arg):
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

    def forward_level(frontier):
        """(live forward children, forward children, target children) of one level."""
        out = search.expand_frontier(v, frontier)
        ch, par = out["children"], out["parent"]
        keep = (ch.fields()["path_len"] > frontier.fields()["path_len"][par]).nonzero().squeeze(1)
        ch, flags = ch.select(keep), out["flags"][keep]
        return ch.select(((flags & 3) == 0).nonzero().squeeze(1)), len(ch), ch.select(((flags & 1) != 0).nonzero().squeeze(1))

    frontier = v.snapshot()
    for _ in range(a.depth):
        frontier = forward_level(frontier)[0]
    distinct = len(frontier)
    roots = frontier.select(torch.arange(a.roots, device=v.device) % distinct)
    M, info, rb, dev = a.roots, roots.info, roots.info.record_bytes, v.device
    row = {"path": path, "roots": M, "distinct_roots": distinct, "root_depth": a.depth, "record_bytes": rb,
           "runs": a.calls}
    stream = torch.cuda.current_stream(dev)
    v._stream()
    if path == "dfs":
        budget = int(arg)
        state = torch.zeros(M, dtype=torch.int32, device=dev)
        counts = torch.zeros((M, _lib.DFS_COUNTERS), dtype=torch.int64, device=dev)
        first = torch.zeros((M, rb), dtype=torch.uint8, device=dev)
        status = torch.zeros(M, dtype=torch.uint8, device=dev)
        cursor = torch.empty((M, rb), dtype=torch.uint8, device=dev)
        times = []
        for r in range(WARM + a.calls):
            state.zero_(), counts.zero_(), first.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            v.core.dfs_device(info, roots.records.data_ptr(), M, budget, state.data_ptr(), status.data_ptr(),
                              counts.data_ptr(), cursor.data_ptr(), first.data_ptr())
            e1.record(stream)
            e1.synchronize()
            if r >= WARM:
                times.append(e0.elapsed_time(e1) * 1e3)
        v.core.sync()
        c = counts.sum(0).cpu().tolist()
        nodes = c[_lib.DFS_NODES]
        st = torch.bincount(status.to(torch.int64), minlength=5).cpu().tolist()
        row.update(budget=budget, nodes=nodes, counters=dict(zip(_lib.DFS_COUNTER_NAMES, c)), status_0_to_4=st)
    else:
        levels = int(arg)
        times, nodes, sizes_ = [], 0, []
        for r in range(WARM + a.calls):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            cur, nodes, sizes_, audited = roots, 0, [], 0
            for _ in range(levels):
                if not len(cur):
                    break
                cur, kept, targets = forward_level(cur)
                if len(targets):
                    v.audit_records(targets)
                    audited += len(targets)
                nodes += kept
                sizes_.append(kept)
                if 4 * len(cur) > 1 << 22:
                    break
            torch.cuda.synchronize(dev)
            if r >= WARM:
                times.append((time.perf_counter() - t0) * 1e6)
        row.update(levels=len(sizes_), level_nodes=sizes_, nodes=nodes, audited=audited)
    med = float(np.median(times))
    row.update(median_us=round(med, 2), p10_us=round(float(np.percentile(times, 10)), 2),
               p90_us=round(float(np.percentile(times, 90)), 2), nodes_per_second=round(nodes / (med * 1e-6), 1),
               device=torch.cuda.get_device_name(0))
    v.close()
    print("ROW " + json.dumps(row), flush=True)


if a.worker:
    worker(a.worker[0], a.worker[1])
    sys.exit(0)

rows = []
for path, arg in [("dfs", str(b)) for b in a.budgets] + [("levels", str(a.levels))]:
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", path, arg,
           "--calls", str(a.calls), "--roots", str(a.roots), "--depth", str(a.depth), "--puzzles", str(a.puzzles)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    line = next((ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")), None)
    if p.returncode != 0 or line is None:
        sys.exit(f"{path} {arg}: the GPU step ended with status {p.returncode}; nothing more is run")
    row = json.loads(line[4:])
    rows.append(row)
    print(f"{path:6s} {arg:>5s}: {row['median_us']:12.2f} us  nodes {row['nodes']:12d}  "
          f"{row['nodes_per_second']:.4g} nodes/s", flush=True)

device = rows[0].pop("device")
for r in rows[1:]:
    r.pop("device")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump({"device": device, "timing": f"median of {a.calls} runs after {WARM} warm-up runs; dfs: device events "
               "around one launch; levels: wall time of the loop between two device synchronisations", "rows": rows},
              f, indent=1)
print("wrote", a.out)
