#!/usr/bin/env python3
"""Device time of sparc_mcts_device against the same UCT written with the calls that existed before it.

Workload: the c3 bench pool (7x7, one word, traceback, max_steps 2000), M roots (default 65,536: the
reset states of M puzzles, cycling through the pool), `--sims` simulations (64) on fresh trees, rollouts
of at most `--horizon` steps (64), forward only, arenas of sims + 1 nodes, the default UCT tables.

The composed path is what a caller of the parent commit writes: per simulation round, for all M trees
at once, the descent by score over node statistics kept in torch tensors (one gather and one argmax per
level, a host test per level for "does any tree still descend"), one sparc_expand_device on the chosen
leaves' records and the gather of the child of the lowest untried action, one sparc_playout_device
(K = 1) from the new inner nodes, and the backup as one scatter per level.  It keeps every node's record
(M * cap records), so its descent takes no step.  Its rollouts draw from another stream (playout g of a
launch draws with id0 + g, not j * 2^32 + s), so its trees are not the kernel's: the same algorithm on
the same roots, compared by node and win totals, not byte for byte.

Each path is timed with device events (the composed one: wall time around a final synchronise, since it
synchronises inside) after a warm-up, alternating; the median of `--calls` rounds is reported.  Runs in
a child process under `timeout`; a failure ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 2

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=7, help="timed rounds (each path once per round)")
ap.add_argument("--roots", type=int, default=65536)
ap.add_argument("--sims", type=int, default=64)
ap.add_argument("--horizon", type=int, default=64)
ap.add_argument("--puzzles", type=int, default=1024)
ap.add_argument("--limit", type=int, default=420, help="seconds allowed to the measurement")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mcts", "prof_mcts.json"))
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
    from sparc_gym_amd.snapshot import Snapshot
    from sparc_gym_amd.vec_env import uct_tables

    sizes, full, tb, _ = bench.CONFIGS["c3"]
    proc = process_puzzles(synthetic.make_puzzles(a.puzzles, seed=0, sizes=sizes, full_properties=full))
    v = SPaRCVecEnv(4, processed=proc, table=pack_table(proc), traceback=tb, max_steps=2000, observation="compact")
    M, S, L, cap, dev = a.roots, a.sims, a.horizon, a.sims + 1, v.device
    snap = v.roots(np.arange(M) % len(proc))
    info, rb, roots = snap.info, snap.info.record_bytes, snap.records
    ep_h, ec_h = uct_tables(1.0)
    ep, ec = torch.from_numpy(ep_h).to(dev), torch.from_numpy(ec_h).to(dev)
    T = len(ep_h)
    ar = torch.arange(M, device=dev)
    NONE = _lib.MCTS_NO_CHILD

    # ---- the kernel
    nodes = torch.empty((M, cap, 16), dtype=torch.int32, device=dev)
    count = torch.zeros(M, dtype=torch.int32, device=dev)
    win = torch.zeros((M, rb), dtype=torch.uint8, device=dev)
    wsteps = torch.full((M,), -1, dtype=torch.int32, device=dev)
    status = torch.empty(M, dtype=torch.uint8, device=dev)
    done = torch.empty(M, dtype=torch.int32, device=dev)

    def kernel():
        v.core.mcts_device(info, roots.data_ptr(), M, S, L, ep.data_ptr(), ec.data_ptr(), T, cap, nodes.data_ptr(),
                           count.data_ptr(), status.data_ptr(), done.data_ptr(), win.data_ptr(), wsteps.data_ptr(),
                           seed=1, flags=_lib.PLAYOUT_FORWARD)

    # ---- the composed UCT: node statistics and records in torch tensors
    def composed():
        i64 = dict(dtype=torch.int64, device=dev)
        parent, action = torch.zeros((M, cap), **i64), torch.zeros((M, cap), **i64)
        kind, code_of = torch.zeros((M, cap), **i64), torch.zeros((M, cap), **i64)
        visits, wins = torch.zeros((M, cap), **i64), torch.zeros((M, cap), **i64)
        child, n, w = (torch.zeros((M, cap, 4), **i64) for _ in range(3))
        recs = torch.empty((M, cap, rb), dtype=torch.uint8, device=dev)
        recs[:, 0] = roots
        ex = v.expand(snap)
        root_moves = ex["legal_mask"].to(torch.int64)              # a reset state has no pop
        bit = 1 << torch.arange(4, device=dev)
        child[:, 0] = torch.where((root_moves[:, None] & bit) != 0, 0, NONE)
        cnt = torch.ones(M, **i64)
        for s in range(S):
            cur = torch.zeros(M, **i64)
            while True:                                            # the descent, one level per trip
                ch = child[ar, cur]
                stop = (ch == 0).any(1) | (kind[ar, cur] != 0)
                if bool(stop.all()):
                    break
                nn = n[ar, cur].clamp(min=1)
                score = w[ar, cur].float() / nn.float() + ep[visits[ar, cur].clamp(max=T - 1), None] * ec[nn.clamp(max=T - 1)]
                score = torch.where(ch == NONE, -torch.inf, score)
                cur = torch.where(stop, cur, ch[ar, score.argmax(1)])
            grow = (kind[ar, cur] == 0) & (cnt < cap)              # every such leaf has an untried action
            act = (child[ar, cur] == 0).int().argmax(1)
            out = v.expand(Snapshot(recs[ar, cur], info))
            f = out["flags"][ar, act].to(torch.int64)
            step_code = out["reward_code"][ar, act].to(torch.int64)
            moves = ((f >> 2) & 15) & ~(1 << (act ^ 2))            # forward moves: legal without the pop
            k = torch.where(f & 1 != 0, 1, torch.where(f & 2 != 0, 2, torch.where(moves == 0, 3, 0)))
            new = torch.where(grow, cnt, 0)
            kid = out["children"].records[4 * ar + act]
            g = grow.nonzero().squeeze(1)
            recs[g, new[g]] = kid[g]
            parent[g, new[g]], action[g, new[g]], kind[g, new[g]], code_of[g, new[g]] = cur[g], act[g], k[g], step_code[g]
            child[g, new[g]] = torch.where((k[g, None] == 0) & ((moves[g, None] & bit) != 0), 0, NONE)
            child[g, cur[g], act[g]] = new[g]
            po = v.playout(Snapshot(kid, info), 1, L, seed=1, id0=s * M, forward_only=True, stats=False)
            rolled = grow & (k == 0) & (po["steps"][:, 0] > 0)
            leaf = torch.where(grow, new, cur)
            last = torch.where(rolled, po["reward_code"][:, 0].to(torch.int64), code_of[ar, leaf])
            won = (last == 100).to(torch.int64)
            cnt = cnt + grow
            at, up = leaf, torch.ones(M, dtype=torch.bool, device=dev)
            while bool(up.any()):                                  # the backup, one level per trip
                u = up.nonzero().squeeze(1)
                visits[u, at[u]] += 1
                wins[u, at[u]] += won[u]
                up = up & (at != 0)
                u = up.nonzero().squeeze(1)
                n[u, parent[u, at[u]], action[u, at[u]]] += 1
                w[u, parent[u, at[u]], action[u, at[u]]] += won[u]
                at = torch.where(up, parent[ar, at], at)
        return int(cnt.sum()), int(wins[:, 0].sum()), int(visits[:, 0].sum())

    v._stream()
    stream = torch.cuda.current_stream(dev)

    def timed_kernel():
        count.zero_()
        wsteps.fill_(-1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        kernel()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def timed_composed():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        box["composed"] = composed()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    box = {}
    times = {"kernel": [], "composed": []}
    for r in range(WARM + a.calls):
        for name, f in (("kernel", timed_kernel), ("composed", timed_composed)):
            t = f()
            if r >= WARM:
                times[name].append(t)
    v.core.sync()
    k_nodes, k_visits = int(count.sum()), int(nodes[:, 0, 1].sum())
    k_wins = int(nodes[:, 0, 2].sum())
    med = {k: float(np.median(t)) for k, t in times.items()}
    row = {"roots": M, "sims": S, "horizon": L, "cap": cap, "puzzles": a.puzzles, "rounds": a.calls,
           "status_done": int((status == _lib.MCTS_DONE).sum()), "device": torch.cuda.get_device_name(0),
           "kernel": {"median_us": round(med["kernel"], 1), "p10_us": round(float(np.percentile(times["kernel"], 10)), 1),
                      "p90_us": round(float(np.percentile(times["kernel"], 90)), 1), "launches": 1,
                      "nodes": k_nodes, "root_wins": k_wins, "simulations": k_visits,
                      "simulations_per_s": round(k_visits / (med["kernel"] * 1e-6), 1)},
           "composed": {"median_us": round(med["composed"], 1),
                        "p10_us": round(float(np.percentile(times["composed"], 10)), 1),
                        "p90_us": round(float(np.percentile(times["composed"], 90)), 1),
                        "per_round": "1 expand + 1 playout + torch bookkeeping, a host test per tree level",
                        "nodes": box["composed"][0], "root_wins": box["composed"][1], "simulations": box["composed"][2],
                        "simulations_per_s": round(box["composed"][2] / (med["composed"] * 1e-6), 1)},
           "kernel_vs_composed": round(med["kernel"] / med["composed"], 5)}
    v.close()
    print("ROW " + json.dumps(row), flush=True)


if a.worker:
    worker()
    sys.exit(0)

cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", "--calls", str(a.calls),
       "--roots", str(a.roots), "--sims", str(a.sims), "--horizon", str(a.horizon), "--puzzles", str(a.puzzles)]
p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
line = next((ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")), None)
if p.returncode != 0 or line is None:
    sys.exit(f"the GPU step ended with status {p.returncode}; nothing more is run")
row = json.loads(line[4:])
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump({"timing": "kernel: device events around one launch on fresh trees; composed: wall time around the whole "
               f"loop, synchronised at both ends; medians of alternating rounds after {WARM} warm-up rounds", "row": row},
              f, indent=1)
print(json.dumps(row, indent=1))
print("wrote", a.out)
