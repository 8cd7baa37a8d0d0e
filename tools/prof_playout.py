#!/usr/bin/env python3
"""Device time of sparc_playout_device against the composed path it replaces.

Workload: the c3 bench pool (7x7, one word, traceback, max_steps 2000), M = 1,024 and 4,096 roots
(the reset states of M puzzles, cycling through the pool), K = 64 playouts each (65,536 and 262,144
playouts), horizon L = 64, in two modes: forward-only (SPARC_PLAYOUT_FORWARD) and all legal moves.

The composed path is the only one the parent commit offers for the same result: L rounds of
sparc_expand_device on the M * K current records plus the gather of the chosen child, every entry
point unchanged since that commit.  It is given its actions for nothing: they are the trace the
kernel wrote, so a round is the expand launch, the index 4 * g + a, the row gather and the select
that keeps an ended playout's record, all on the GPU in torch.  A real caller also has to compute
the draws and the pop per ply, so the composed figure is a lower bound.  Its final records are
compared with the kernel's at the timed sizes.
The kernel is timed twice: with every output (trace and final records included: what the composed
path produces), and with the root statistics alone (what a flat Monte-Carlo search reads).

Each path is timed with device events on the context's stream after a warm-up, in rounds that
alternate the three on the same box; the median of `--calls` rounds is reported with the medians of
the four quarters of the rounds, whose spread for the composed path is the margin within which a
difference counts.  Every shape runs in a child process of its own under `timeout`; the first one
that fails or overruns ends the run."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 5
MODES = {"forward": 1, "all_legal": 0}

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30, help="timed rounds (each path once per round)")
ap.add_argument("--roots", type=int, nargs="+", default=[1024, 4096])
ap.add_argument("--playouts", type=int, default=64, help="K, playouts per root")
ap.add_argument("--horizon", type=int, default=64, help="L, steps at most")
ap.add_argument("--puzzles", type=int, default=1024)
ap.add_argument("--limit", type=int, default=240, help="seconds allowed to one shape")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "playout", "prof_playout.json"))
ap.add_argument("--worker", nargs=2, metavar=("MODE", "M"), help=argparse.SUPPRESS)
a = ap.parse_args()


def worker(mode, M):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "sparc-gym_amd"))
    import numpy as np
    import torch

    import bench
    from sparc_gym_amd import SPaRCVecEnv, synthetic
    from sparc_gym_amd.puzzles import pack_table, process_puzzles

    sizes, full, tb, _ = bench.CONFIGS["c3"]
    proc = process_puzzles(synthetic.make_puzzles(a.puzzles, seed=0, sizes=sizes, full_properties=full))
    table = pack_table(proc)
    v = SPaRCVecEnv(M, processed=proc, table=table, traceback=tb, max_steps=2000, observation="compact")
    v.reset(options={"puzzle_index": np.arange(M) % len(proc)})
    K, L, flags, dev = a.playouts, a.horizon, MODES[mode], v.device
    MK = M * K
    snap = v.snapshot()
    info, rb = snap.info, snap.info.record_bytes
    roots = snap.records
    start = roots.repeat_interleave(K, dim=0).contiguous()          # record g // K, for the composed path
    g4 = 4 * torch.arange(MK, device=dev)

    i8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)   # noqa: E731
    code, flg, first, end, trace, final = i8(MK), i8(MK), i8(MK), i8(MK), i8(L, MK), i8(MK, rb)
    steps = torch.empty(MK, dtype=torch.int16, device=dev)
    ret = torch.empty(MK, dtype=torch.int32, device=dev)
    stats = torch.zeros((M, 4, 4), dtype=torch.int32, device=dev)

    def playout_all():
        v.core.playout_device(info, roots.data_ptr(), M, K, L, seed=1, flags=flags, d_code=code.data_ptr(),
                              d_flags=flg.data_ptr(), d_steps=steps.data_ptr(), d_first=first.data_ptr(),
                              d_end=end.data_ptr(), d_return=ret.data_ptr(), d_trace=trace.data_ptr(),
                              d_final=final.data_ptr(), d_stats=stats.data_ptr())

    def playout_stats():
        v.core.playout_device(info, roots.data_ptr(), M, K, L, seed=1, flags=flags, d_stats=stats.data_ptr())

    children = i8(4 * MK, rb)
    box = {}

    def composed():
        cur = start
        for t in range(L):
            v.core.expand_device(info, cur.data_ptr(), MK, children.data_ptr())
            act = trace[t].to(torch.int64)
            took = act < 4
            cur = torch.where(took[:, None], children[g4 + torch.where(took, act, 0)], cur)
        box["final"] = cur

    v._stream()
    playout_all()                                                    # the trace the composed path replays
    v.core.sync()
    ops = {"playout_all": playout_all, "playout_stats": playout_stats, "composed": composed}
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
    v.core.sync()
    equal = bool(torch.equal(box["final"], final))
    n = (steps.to(torch.int64) & 0xFFFF)
    ends = torch.bincount(end.to(torch.int64), minlength=6).cpu().tolist()
    med = {k: float(np.median(t)) for k, t in times.items()}
    quarters = {k: [float(np.median(c)) for c in np.array_split(np.asarray(t), 4)] for k, t in times.items()}
    spread = max(quarters["composed"]) - min(quarters["composed"])
    # the steps a wave runs: the longest playout of each 64 lanes
    wave_steps = n[:MK // 64 * 64].reshape(-1, 64).max(1).values.double().mean().item()
    row = {"mode": mode, "roots": M, "playouts_per_root": K, "playouts": MK, "horizon": L, "record_bytes": rb,
           "rounds": a.calls, "final_records_equal": equal, "mean_playout_steps": round(n.double().mean().item(), 3),
           "mean_steps_of_a_wave": round(wave_steps, 3), "end_reasons_0_to_5": ends,
           "wins": int((code.view(torch.int8) == 100).sum()),
           "all_vs_composed": round(med["playout_all"] / med["composed"], 4),
           "stats_vs_composed": round(med["playout_stats"] / med["composed"], 4),
           "composed_quarter_median_spread_us": round(spread, 2)}
    for k in ops:
        t = times[k]
        row[k] = {"median_us": round(med[k], 2), "p10_us": round(float(np.percentile(t, 10)), 2),
                  "p90_us": round(float(np.percentile(t, 90)), 2),
                  "quarter_medians_us": [round(q, 2) for q in quarters[k]],
                  "launches": 1 if k != "composed" else f"{L} expand + {6 * L} torch"}
    row["device"] = torch.cuda.get_device_name(0)
    v.close()
    print("ROW " + json.dumps(row), flush=True)


if a.worker:
    worker(a.worker[0], int(a.worker[1]))
    sys.exit(0)

rows = []
for mode in MODES:
    for M in a.roots:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", mode, str(M),
               "--calls", str(a.calls), "--puzzles", str(a.puzzles), "--playouts", str(a.playouts),
               "--horizon", str(a.horizon)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")), None)
        if p.returncode != 0 or line is None:
            sys.exit(f"{mode} M={M}: the GPU step ended with status {p.returncode}; nothing more is run")
        row = json.loads(line[4:])
        rows.append(row)
        print(f"{mode:9s} playouts={row['playouts']:7d} all outputs {row['playout_all']['median_us']:9.2f} us  stats only "
              f"{row['playout_stats']['median_us']:9.2f} us  composed {row['composed']['median_us']:10.2f} us  ratios "
              f"{row['all_vs_composed']:.4f} {row['stats_vs_composed']:.4f}  mean steps {row['mean_playout_steps']:.2f} "
              f"(wave {row['mean_steps_of_a_wave']:.2f})  equal {row['final_records_equal']}", flush=True)

device = rows[0].pop("device")
for r in rows[1:]:
    r.pop("device")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump({"device": device, "timing": "device events around one path, median; the three paths alternate in rounds "
               f"after {WARM} warm-up rounds", "composed": "L rounds of sparc_expand_device + gather of the chosen child, "
               "actions taken from the kernel's trace (a lower bound of the composed path)", "rows": rows}, f, indent=1)
print("wrote", a.out)
bad = [r for r in rows if not r["final_records_equal"]]
if bad:
    sys.exit("the two paths' final records differ at: " + ", ".join(f"{r['mode']} M={r['roots']}" for r in bad))
