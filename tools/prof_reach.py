#!/usr/bin/env python3
"""Device time of sparc_reach_records_device against the project's own plane writer and against the
only way the parent commit offers to the same numbers.

Workload: that of profiles/observe/ (the c3 bench pool, 7x7, one word, traceback, max_steps 2000;
the records are the `states` of the profiles/replay/ workload, the zeroed ones dropped, cut to a
whole number of 65,536-record chunks), at all of the records and at the first 65,536 alone.  Paths:

  (a) reach without the plane          dist, action_dist, live, size: 7 bytes per record
  (b) reach with the plane             + one uint8 plane per record
  (c) observe with uint8 planes        the project's own launch that reads the same records and
                                       writes planes of the same size (two of them): the floor (b)
                                       is read against
  (d) torch flood                      written here, not in the product: the uint8 `visited` planes,
                                       the puzzle index and the agent of (c), then tensor ops (shift,
                                       mask, compare in a loop) until nothing changes; (c)'s time is
                                       not counted in it

Each path is timed with device events on the context's stream after 5 warm-up rounds, in rounds that
alternate the paths; median, p10 and p90 of `--calls` rounds.  Bytes per launch are computed from the
shapes.  Also recorded: that (b)'s outputs equal (d)'s in every byte, and the node counts of
search.solve_by_rules with and without `prune` on the pool's first 64 puzzles.  Writes
prof_reach.json and, next to it, README.md (the table; a "## Reading" section a person added is
kept).  The measurement runs in a child process under `timeout`; if it fails or overruns nothing
more is run."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 5
CHUNK = 65536

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30, help="timed rounds (each path once per round)")
ap.add_argument("--roots", type=int, default=1024)
ap.add_argument("--per-root", type=int, default=64, help="sequences per root")
ap.add_argument("--horizon", type=int, default=64, help="L, actions at most")
ap.add_argument("--puzzles", type=int, default=1024)
ap.add_argument("--search-puzzles", type=int, default=64)
ap.add_argument("--limit", type=int, default=400, help="seconds allowed to the measurement")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reach", "prof_reach.json"))
ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
a = ap.parse_args()
PATHS = ("reach", "reach_plane", "observe_u8", "torch_flood")


def worker():
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "sparc-gym_amd"))
    import numpy as np
    import torch

    import bench
    from sparc_gym_amd import SPaRCVecEnv, _lib, search, synthetic
    from sparc_gym_amd.puzzles import pack_table, process_puzzles

    sizes, full, tb, _ = bench.CONFIGS["c3"]
    proc = process_puzzles(synthetic.make_puzzles(a.puzzles, seed=0, sizes=sizes, full_properties=full))
    table = pack_table(proc)
    v = SPaRCVecEnv(1, processed=proc, table=table, traceback=tb, max_steps=2000, observation="compact")
    R, K, L, dev = a.roots, a.per_root, a.horizon, v.device
    roots = v.roots(np.arange(R) % len(proc))                       # no env is reset
    po = v.playout(roots, K, L, seed=1, trace=True, final=False, stats=False)
    start = roots.select(torch.arange(R * K, device=dev) // K)
    out = v.replay(start, po["trace"].reshape(L, R * K).contiguous(), lengths=po["steps"].reshape(R * K),
                   stop_done=True, final=False, states=True)
    st = out["states"]
    snap = st.select(st.records[:, 2] != 0)                         # path length 0: a zeroed record
    M = len(snap) // CHUNK * CHUNK
    snap = snap.select(torch.arange(M, device=dev))
    del out, st, po
    info, rec = snap.info, snap.records
    X, Y, XY = v.x_dim, v.y_dim, v.x_dim * v.y_dim

    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)   # noqa: E731
    o = {"dist": u8(M), "action_dist": u8(M, 4), "live": u8(M), "size": u8(M), "plane": u8(M, X, Y)}
    vis, agent = u8(M, X, Y), u8(M, X, Y)
    pidx, loc = torch.empty(M, dtype=torch.int32, device=dev), torch.empty((M, 2), dtype=torch.int32, device=dev)
    legal = u8(M)

    def reach(m, plane):
        v.core.reach_records_device(info, rec.data_ptr(), m, X, Y, d_dist=o["dist"].data_ptr(),
                                    d_action_dist=o["action_dist"].data_ptr(), d_live=o["live"].data_ptr(),
                                    d_size=o["size"].data_ptr(), d_plane=o["plane"].data_ptr() if plane else None)

    def observe(m):
        v.core.observe_records_device(info, rec.data_ptr(), m, _lib.OBS_U8, X, Y, 0, d_visited=vis.data_ptr(),
                                      d_agent=agent.data_ptr(), d_puzzle=pidx.data_ptr(), d_loc=loc.data_ptr(),
                                      d_legal=legal.data_ptr())

    # (d): the static planes of the pool, then shifts and masks on [m, X, Y] tensors
    open_p = torch.zeros((len(proc), X, Y), dtype=torch.bool, device=dev)
    tgt = torch.zeros((len(proc), 2), dtype=torch.int64, device=dev)
    for q, p in enumerate(proc):
        g = np.zeros((X, Y), bool)
        g[:p["x_size"], :p["y_size"]] = np.asarray(p["obs_array"]["gaps"])[:p["x_size"], :p["y_size"]] == 0
        open_p[q] = torch.from_numpy(g).to(dev)
        tgt[q] = torch.tensor([int(c) for c in p["target_location"]], device=dev)
    DX, DY = (1, 0, -1, 0), (0, -1, 0, 1)
    flood = {}

    def torch_flood(m):
        q = pidx[:m].to(torch.int64)
        free = open_p[q] & (vis[:m] == 0)
        rows = torch.arange(m, device=dev)
        Rb = torch.zeros((m, X, Y), dtype=torch.bool, device=dev)
        Rb[rows, tgt[q, 0], tgt[q, 1]] = True
        Rb &= free
        D = torch.full((m, X, Y), 255, dtype=torch.uint8, device=dev)
        D[Rb] = 0
        k = 0
        while True:
            nb = torch.zeros_like(Rb)
            nb[:, 1:] |= Rb[:, :-1]
            nb[:, :-1] |= Rb[:, 1:]
            nb[:, :, 1:] |= Rb[:, :, :-1]
            nb[:, :, :-1] |= Rb[:, :, 1:]
            new = nb & free & ~Rb
            if not bool(new.any()):
                break
            k += 1
            D[new] = k
            Rb |= new
        x, y = loc[:m, 0].to(torch.int64), loc[:m, 1].to(torch.int64)
        ad = torch.full((m, 4), 255, dtype=torch.int64, device=dev)
        for d in range(4):
            nx, ny = x + DX[d], y + DY[d]
            inb = (nx >= 0) & (nx < X) & (ny >= 0) & (ny < Y)
            dn = D[rows, nx.clamp(0, X - 1), ny.clamp(0, Y - 1)].to(torch.int64)
            ad[:, d] = torch.where(inb & (dn != 255), dn + 1, ad[:, d])
        live = sum((ad[:, d] != 255).to(torch.int64) << d for d in range(4))
        dist = torch.where((x == tgt[q, 0]) & (y == tgt[q, 1]), torch.zeros_like(x), ad.min(dim=1).values)
        flood[m] = {"dist": dist.to(torch.uint8), "action_dist": ad.to(torch.uint8), "live": live.to(torch.uint8),
                    "size": Rb.sum(dim=(1, 2)).to(torch.uint8), "plane": D}

    def forward_legal(m):
        """The legal actions without the traceback pop, from (c)'s outputs (not timed)."""
        q, rows = pidx[:m].to(torch.int64), torch.arange(m, device=dev)
        free = open_p[q] & (vis[:m] == 0)
        x, y = loc[:m, 0].to(torch.int64), loc[:m, 1].to(torch.int64)
        fwd = torch.zeros(m, dtype=torch.uint8, device=dev)
        for d in range(4):
            nx, ny = x + DX[d], y + DY[d]
            inb = (nx >= 0) & (nx < X) & (ny >= 0) & (ny < Y)
            fwd |= (inb & free[rows, nx.clamp(0, X - 1), ny.clamp(0, Y - 1)]).to(torch.uint8) << d
        return fwd

    v._stream()
    stream = torch.cuda.current_stream(dev)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        f()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    row = {"record_bytes": info.record_bytes, "x_dim": X, "y_dim": Y, "rounds": a.calls, "sizes": {}}
    W = table.words
    for m in (CHUNK, M):
        ops = {"reach": lambda: reach(m, False), "reach_plane": lambda: reach(m, True), "observe_u8": lambda: observe(m),
               "torch_flood": lambda: torch_flood(m)}
        observe(m)                                                   # (d) starts from (c)'s outputs
        times = {k: [] for k in ops}
        for r in range(WARM + a.calls):
            for name, f in ops.items():
                t = timed(f)
                if r >= WARM:
                    times[name].append(t)
        v.core.sync()
        equal = all(bool(torch.equal(o[k][:m], flood[m][k])) for k in o)
        byt = {"reach": (16 + 8 * W, 7), "reach_plane": (16 + 8 * W, 7 + XY),
               "observe_u8": (16 + 8 * W + (4 if tb else 0), 2 * XY + 13), "torch_flood": (None, None)}
        s = {"records": m, "reach_plane_equals_torch_flood": equal,
             "lost": int((o["dist"][:m] == 255).sum()), "on_target": int((o["dist"][:m] == 0).sum()),
             "max_dist": int(o["dist"][:m][o["dist"][:m] != 255].max()),
             "pruned_actions": int(((forward_legal(m) & ~o["live"][:m]) != 0).sum())}
        for k in ops:
            t = times[k]
            med = float(np.median(t))
            rd, wr = byt[k]
            s[k] = {"median_us": round(med, 2), "p10_us": round(float(np.percentile(t, 10)), 2),
                    "p90_us": round(float(np.percentile(t, 90)), 2),
                    "bytes_read": rd and rd * m, "bytes_written": wr and wr * m,
                    "gb_per_s": rd and round((rd + wr) * m / med * 1e-3, 1)}
        s["reach_vs_observe"] = round(s["reach"]["median_us"] / s["observe_u8"]["median_us"], 4)
        s["reach_plane_vs_observe"] = round(s["reach_plane"]["median_us"] / s["observe_u8"]["median_us"], 4)
        s["reach_plane_vs_torch_flood"] = round(s["reach_plane"]["median_us"] / s["torch_flood"]["median_us"], 6)
        s["reach_plane_p90_below_torch_flood_p10"] = s["reach_plane"]["p90_us"] < s["torch_flood"]["p10_us"]
        row["sizes"][str(m)] = s
        flood.clear()
    # the search: node counts with and without prune
    S = a.search_puzzles
    w = SPaRCVecEnv(S, processed=proc[:S], traceback=tb, autoreset="none", observation="compact", max_steps=2000)
    plain = search.solve_by_rules(w, np.arange(S))
    pruned = search.solve_by_rules(w, np.arange(S), prune=True)
    w.core.sync()
    same = all(plain["paths"][r] == pruned["paths"][r] and np.array_equal(plain["bits"][r], pruned["bits"][r])
               for r in range(S))
    row["search"] = {"puzzles": S, "nodes": int(plain["nodes"].sum()), "nodes_pruned": int(pruned["nodes"].sum()),
                     "ratio": round(float(pruned["nodes"].sum() / plain["nodes"].sum()), 4),
                     "paths": sum(len(p) for p in plain["paths"]), "same_paths_and_bits": bool(same)}
    row["device"] = torch.cuda.get_device_name(0)
    v.close()
    w.close()
    print("ROW " + json.dumps(row), flush=True)


NAMES = {"reach": "(a) `reach`, no plane", "reach_plane": "(b) `reach` with the plane",
         "observe_u8": "(c) `observe`, uint8 planes", "torch_flood": "(d) torch flood of (c)'s planes"}


def readme(row, device):
    lines = [
        "# profiles/reach — target reachability and distance maps of state records", "",
        f"- `prof_reach.json`: `python tools/prof_reach.py` on one MI355X (torch names it \"{device}\"). Device events around one path,",
        f"  median of {row['rounds']} rounds after {WARM} warm-up rounds, the paths alternating in one process. Workload: that of",
        f"  `profiles/observe/` (the c3 pool, 7×7, traceback; records of {row['record_bytes']} B, planes {row['x_dim']}×{row['y_dim']}).",
        "- (c) is the project's own launch that reads the same records and writes planes of the same size (two of",
        "  them). (d) is the only way the parent commit offers to the same numbers, written inside the tool: the",
        "  uint8 `visited` planes, puzzle index and agent of (c), then torch tensor ops (shift, mask, compare in a",
        "  loop with one host read per trip) until nothing changes. (c)'s time is not counted in (d).", ""]
    for m, s in row["sizes"].items():
        lines += [f"## {int(m):,} records", "",
                  "| path | median | p10 .. p90 | bytes read | bytes written | read + written / time |", "|---|---|---|---|---|---|"]
        for k in PATHS:
            r = s[k]
            io = (f"{r['bytes_read']:,} | {r['bytes_written']:,} | {r['gb_per_s']:,.1f} GB/s" if r["bytes_read"]
                  else "not counted | not counted | not counted")
            lines.append(f"| {NAMES[k]} | {r['median_us']:,.2f} µs | {r['p10_us']:,.2f} .. {r['p90_us']:,.2f} | {io} |")
        lines += ["", f"- (a)/(c) {s['reach_vs_observe']}, (b)/(c) {s['reach_plane_vs_observe']}, (b)/(d) {s['reach_plane_vs_torch_flood']}.",
                  f"- Acceptance ((b)'s p90 below (d)'s p10): {s['reach_plane_p90_below_torch_flood_p10']}.",
                  f"- (b)'s five outputs equal (d)'s in every byte: {s['reach_plane_equals_torch_flood']}.",
                  f"- Of these records {s['lost']:,} are lost, {s['on_target']:,} stand on the target, {s['pruned_actions']:,} have a legal",
                  f"  action that is not live; the largest distance is {s['max_dist']}.", ""]
    q = row["search"]
    lines += ["## `search.solve_by_rules` with and without `prune`", "",
              f"- The pool's first {q['puzzles']} puzzles, every root at once: {q['nodes']:,} forward-move nodes without `prune`,",
              f"  {q['nodes_pruned']:,} with it ({q['ratio']} of them); {q['paths']:,} paths to the target, the same paths and rule bits in",
              f"  the same order: {q['same_paths_and_bits']}.", ""]
    return "\n".join(lines)


if a.worker:
    worker()
    sys.exit(0)

cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", "--calls", str(a.calls),
       "--puzzles", str(a.puzzles), "--roots", str(a.roots), "--per-root", str(a.per_root), "--horizon", str(a.horizon),
       "--search-puzzles", str(a.search_puzzles)]
p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
line = next((ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")), None)
if p.returncode != 0 or line is None:
    sys.exit(f"the GPU step ended with status {p.returncode}; nothing more is run")
row = json.loads(line[4:])
for m, s in row["sizes"].items():
    for k in PATHS:
        print(f"{m} {k}: {s[k]['median_us']:.2f} us ({s[k]['p10_us']:.2f} .. {s[k]['p90_us']:.2f})", flush=True)
    print(f"{m} (a)/(c) {s['reach_vs_observe']}  (b)/(c) {s['reach_plane_vs_observe']}  (b)/(d) {s['reach_plane_vs_torch_flood']}  "
          f"accepted {s['reach_plane_p90_below_torch_flood_p10']}  equal {s['reach_plane_equals_torch_flood']}", flush=True)
print("search", row["search"], flush=True)
device = row.pop("device")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump({"device": device, "timing": "device events around one path, median; the paths alternate in rounds "
               f"after {WARM} warm-up rounds", "torch_flood": "the uint8 visited planes, puzzle index and agent of observe, then "
               "torch tensor ops (shift, mask, compare) until nothing changes; observe's time not counted", "rows": [row]},
              f, indent=1)
# the README's table is rewritten; what a person wrote below "## Reading" stays
path = os.path.join(os.path.dirname(os.path.abspath(a.out)), "README.md")
kept = open(path).read() if os.path.exists(path) else ""
kept = kept[kept.index("\n## Reading"):] if "\n## Reading" in kept else ""
with open(path, "w") as f:
    f.write(readme(row, device) + kept)
print("wrote", a.out)
if not all(s["reach_plane_equals_torch_flood"] for s in row["sizes"].values()):
    sys.exit("the paths' outputs differ")
