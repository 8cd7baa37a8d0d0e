#!/usr/bin/env python3
"""Device time of sparc_replay_device against the chained path it replaces.

Workload: the c3 bench pool (7x7, one word, traceback, max_steps 2000), 65,536 sequences of 64
actions from the roots of profiles/playout/ (the reset states of M = 1,024 puzzles, 64 sequences
each).  The actions are the trace of one sparc_playout_device launch from the same roots (all legal
moves), so the work is that of profiles/playout/: a sequence has its playout's number of actions and
ends with the step that ends its episode (SPARC_REPLAY_STOP_DONE).

The chained path is the only one the parent commit offers for given actions without an env: L
rounds of sparc_expand_device on the current records plus the gather of the chosen child, all on
the GPU in torch (the index 4 * g + a, the row gather, the select that keeps an ended sequence's
record).  It produces the final records only; per-step codes and flags would cost it two more gathers
a round, so its figure is a lower bound.  Its final records are compared with the kernel's.
The kernel is timed in three forms: the per-sequence outputs and the final records (what the chained
path produces); those plus the per-step codes and flags; and those plus the record after every step
(the STATES instantiation), whose stores are L * M records.

Each path is timed with device events on the context's stream after a warm-up, in rounds that
alternate the four; the median of `--calls` rounds is reported with the medians of the four quarters
of the rounds, whose spread for the chained path is the margin within which a difference counts.
The measurement runs in a child process under `timeout`; if it fails or overruns nothing more is run."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 5

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30, help="timed rounds (each path once per round)")
ap.add_argument("--roots", type=int, default=1024)
ap.add_argument("--per-root", type=int, default=64, help="sequences per root")
ap.add_argument("--horizon", type=int, default=64, help="L, actions at most")
ap.add_argument("--puzzles", type=int, default=1024)
ap.add_argument("--limit", type=int, default=300, help="seconds allowed to the measurement")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "replay", "prof_replay.json"))
ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
a = ap.parse_args()


def worker():
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "sparc-gym_amd"))
    import numpy as np
    import torch

    import bench
    from sparc_gym_amd import SPaRCVecEnv, _lib, synthetic
    from sparc_gym_amd.puzzles import pack_table, process_puzzles

    sizes, full, tb, _ = bench.CONFIGS["c3"]
    proc = process_puzzles(synthetic.make_puzzles(a.puzzles, seed=0, sizes=sizes, full_properties=full))
    table = pack_table(proc)
    v = SPaRCVecEnv(1, processed=proc, table=table, traceback=tb, max_steps=2000, observation="compact")
    R, K, L, dev = a.roots, a.per_root, a.horizon, v.device
    M = R * K
    roots = v.roots(np.arange(R) % len(proc))                       # no env is reset
    info, rb = roots.info, roots.info.record_bytes
    po = v.playout(roots, K, L, seed=1, trace=True, final=True, stats=False)
    trace = po["trace"].reshape(L, M).contiguous()
    lens = po["steps"].reshape(M).to(torch.int32).contiguous()
    start = roots.records.repeat_interleave(K, dim=0).contiguous()  # record g // K
    g4 = 4 * torch.arange(M, device=dev)

    i8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)   # noqa: E731
    code, flg, end, final, scode, sflg = i8(M), i8(M), i8(M), i8(M, rb), i8(L, M), i8(L, M)
    steps, bad = torch.empty(M, dtype=torch.int16, device=dev), torch.empty(M, dtype=torch.int16, device=dev)
    ret = torch.empty(M, dtype=torch.int32, device=dev)
    states = i8(L * M, rb)
    flags = _lib.REPLAY_STOP_DONE

    def replay(**more):
        v.core.replay_device(info, start.data_ptr(), None, M, L, trace.data_ptr(), lens.data_ptr(), flags,
                             d_code=code.data_ptr(), d_flags=flg.data_ptr(), d_steps=steps.data_ptr(),
                             d_end=end.data_ptr(), d_return=ret.data_ptr(), d_bad=bad.data_ptr(),
                             d_final=final.data_ptr(), **more)

    def replay_final():
        replay()

    def replay_per_step():
        replay(d_step_code=scode.data_ptr(), d_step_flags=sflg.data_ptr())

    def replay_states():
        replay(d_step_code=scode.data_ptr(), d_step_flags=sflg.data_ptr(), d_states=states.data_ptr())

    children = i8(4 * M, rb)
    box = {}

    def chained():
        cur = start
        for t in range(L):
            v.core.expand_device(info, cur.data_ptr(), M, children.data_ptr())
            act = trace[t].to(torch.int64)
            took = act < 4
            cur = torch.where(took[:, None], children[g4 + torch.where(took, act, 0)], cur)
        box["final"] = cur

    v._stream()
    ops = {"replay_final": replay_final, "replay_per_step": replay_per_step, "replay_states": replay_states,
           "chained": chained}
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
    n = steps.to(torch.int64) & 0xFFFF
    equal = bool(torch.equal(box["final"], final)) and bool(torch.equal(final, po["final"].records))
    equal = equal and bool(torch.equal(n, lens.to(torch.int64)))
    last = torch.clamp(n - 1, min=0) * M + torch.arange(M, device=dev)
    states_equal = bool(torch.equal(states[last][n > 0], final[n > 0]))
    med = {k: float(np.median(t)) for k, t in times.items()}
    quarters = {k: [float(np.median(c)) for c in np.array_split(np.asarray(t), 4)] for k, t in times.items()}
    wave_steps = n[:M // 64 * 64].reshape(-1, 64).max(1).values.double().mean().item()
    row = {"roots": R, "sequences_per_root": K, "sequences": M, "horizon": L, "record_bytes": rb, "rounds": a.calls,
           "final_records_equal": equal, "last_state_equals_final": states_equal,
           "mean_sequence_steps": round(n.double().mean().item(), 3), "mean_steps_of_a_wave": round(wave_steps, 3),
           "end_reasons_0_to_5": torch.bincount(end.to(torch.int64), minlength=6).cpu().tolist(),
           "final_vs_chained": round(med["replay_final"] / med["chained"], 4),
           "per_step_vs_final": round(med["replay_per_step"] / med["replay_final"], 4),
           "states_vs_per_step": round(med["replay_states"] / med["replay_per_step"], 4),
           "states_bytes_stored": L * M * rb,
           "chained_quarter_median_spread_us": round(max(quarters["chained"]) - min(quarters["chained"]), 2)}
    for k in ops:
        t = times[k]
        row[k] = {"median_us": round(med[k], 2), "p10_us": round(float(np.percentile(t, 10)), 2),
                  "p90_us": round(float(np.percentile(t, 90)), 2),
                  "quarter_medians_us": [round(q, 2) for q in quarters[k]],
                  "launches": 1 if k != "chained" else f"{L} expand + {6 * L} torch"}
    row["device"] = torch.cuda.get_device_name(0)
    v.close()
    print("ROW " + json.dumps(row), flush=True)


if a.worker:
    worker()
    sys.exit(0)

cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", "--calls", str(a.calls),
       "--puzzles", str(a.puzzles), "--roots", str(a.roots), "--per-root", str(a.per_root), "--horizon", str(a.horizon)]
p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
line = next((ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")), None)
if p.returncode != 0 or line is None:
    sys.exit(f"the GPU step ended with status {p.returncode}; nothing more is run")
row = json.loads(line[4:])
print(f"sequences={row['sequences']} final {row['replay_final']['median_us']:.2f} us  per-step "
      f"{row['replay_per_step']['median_us']:.2f} us  states {row['replay_states']['median_us']:.2f} us  chained "
      f"{row['chained']['median_us']:.2f} us  final/chained {row['final_vs_chained']:.4f}  states/per-step "
      f"{row['states_vs_per_step']:.4f}  mean steps {row['mean_sequence_steps']:.2f} (wave "
      f"{row['mean_steps_of_a_wave']:.2f})  equal {row['final_records_equal']} {row['last_state_equals_final']}", flush=True)
device = row.pop("device")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump({"device": device, "timing": "device events around one path, median; the four paths alternate in rounds "
               f"after {WARM} warm-up rounds", "chained": "L rounds of sparc_expand_device + gather of the chosen child "
               "(final records only: a lower bound of the chained path)", "rows": [row]}, f, indent=1)
print("wrote", a.out)
if not (row["final_records_equal"] and row["last_state_equals_final"]):
    sys.exit("the paths' records differ")
