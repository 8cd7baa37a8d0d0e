#!/usr/bin/env python3
"""Device time of sparc_observe_records_device against the chained path it replaces.

Workload: the c3 bench pool (7x7, one word, traceback, max_steps 2000).  The records are the
`states` of the profiles/replay/ workload: 65,536 sequences of at most 64 actions from the roots of
1,024 puzzles, the record after every step; the zeroed records (at and after a sequence's end) are
dropped with Snapshot.select, so no record is refused, and the count is cut to a whole number of
65,536-record chunks for the chained path's sake.  Rows: int32 planes dense (the reference's dtype);
uint8 planes dense; float16 planes into channels (3, 1) of an [M, 8, 7, 7] tensor; and the first
65,536 records alone, int32 dense (the latency of one frontier).

The chained path is the only one the parent commit offers from records to planes: per chunk of
65,536 records sparc_restore_device into a 65,536-env context, sparc_obs_pack_device into the
chunk's planes, and two sparc_copy_state_device (puzzle index, position).  It is int32 only: that
path can produce no other element type, no legal actions and no stride.

Each path is timed with device events on the context's stream after 5 warm-up rounds, in rounds that
alternate the paths; median, p10 and p90 of `--calls` rounds.  Bytes per launch are computed from
the shapes (2 * x_dim * y_dim * element size + 13 written, 16 + 8 * words + 4 read per record; the
stack word is read under traceback for the legal actions).  `--fill-gbs` takes the store bandwidth
tools/stream_bw measured in the same job, for the "of fill" column.  Writes prof_observe.json and,
next to it, README.md (the table; a "## Reading" section a person added is kept).  The measurement
runs in a child process under `timeout`; if it fails or overruns nothing more is run."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 5
CHUNK = 65536
C4_OBSW_GBS = 6765.94   # k_rollout_obsw on c4, profiles/r06/final_bench/bench_c4.log (roofline.achieved)

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30, help="timed rounds (each path once per round)")
ap.add_argument("--roots", type=int, default=1024)
ap.add_argument("--per-root", type=int, default=64, help="sequences per root")
ap.add_argument("--horizon", type=int, default=64, help="L, actions at most")
ap.add_argument("--puzzles", type=int, default=1024)
ap.add_argument("--limit", type=int, default=300, help="seconds allowed to the measurement")
ap.add_argument("--fill-gbs", type=float, default=0.0, help="tools/stream_bw's store bandwidth of this job, GB/s")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "observe", "prof_observe.json"))
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
    roots = v.roots(np.arange(R) % len(proc))                       # no env is reset
    po = v.playout(roots, K, L, seed=1, trace=True, final=False, stats=False)
    start = roots.select(torch.arange(R * K, device=dev) // K)
    out = v.replay(start, po["trace"].reshape(L, R * K).contiguous(), lengths=po["steps"].reshape(R * K),
                   stop_done=True, final=False, states=True)
    st = out["states"]
    live = st.records[:, 2] != 0                                    # path length 0: a zeroed record
    snap = st.select(live)
    M = len(snap) // CHUNK * CHUNK
    snap = snap.select(torch.arange(M, device=dev))
    del out, st, po
    info, rec = snap.info, snap.records
    X, Y, XY = v.x_dim, v.y_dim, v.x_dim * v.y_dim
    C, cv, ca = 8, 3, 1

    e32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)   # noqa: E731
    pidx, loc, legal = e32(M), e32(M, 2), torch.empty(M, dtype=torch.uint8, device=dev)
    planes = {"i32": e32(2, M, X, Y), "u8": torch.empty((2, M, X, Y), dtype=torch.uint8, device=dev)}
    net = torch.zeros((M, C, X, Y), dtype=torch.float16, device=dev)

    def observe(elem, vis, agent, m=M, stride=0):
        v.core.observe_records_device(info, rec.data_ptr(), m, elem, X, Y, stride, d_visited=vis.data_ptr(),
                                      d_agent=agent.data_ptr(), d_puzzle=pidx.data_ptr(), d_loc=loc.data_ptr(),
                                      d_legal=legal.data_ptr())

    w = SPaRCVecEnv(CHUNK, processed=proc, table=table, traceback=tb, max_steps=2000, observation="compact")
    w._stream()
    ch_planes, ch_pidx, ch_pos = e32(2, M, X, Y), e32(M), e32(M)
    flags = torch.empty(CHUNK, dtype=torch.uint8, device=dev)
    rb = info.record_bytes

    def chained():
        for c in range(M // CHUNK):
            lo = c * CHUNK
            w.core.restore_device(info, rec.data_ptr() + lo * rb, CHUNK, None, None, flags.data_ptr())
            w.core.obs_pack_device(ch_planes[0, lo:].data_ptr(), ch_planes[1, lo:].data_ptr(), X, Y)
            w.core.copy_state_device(4, ch_pidx[lo:].data_ptr())
            w.core.copy_state_device(1, ch_pos[lo:].data_ptr())

    ops = {"observe_i32": lambda: observe(_lib.OBS_I32, planes["i32"][0], planes["i32"][1]),
           "observe_u8": lambda: observe(_lib.OBS_U8, planes["u8"][0], planes["u8"][1]),
           "observe_f16_2_of_8_channels": lambda: observe(_lib.OBS_F16, net[:, cv], net[:, ca], stride=C * XY),
           "observe_i32_65536": lambda: observe(_lib.OBS_I32, planes["i32"][0], planes["i32"][1], m=CHUNK),
           "chained_i32": chained}
    elem_bytes = {"observe_i32": 4, "observe_u8": 1, "observe_f16_2_of_8_channels": 2, "observe_i32_65536": 4,
                  "chained_i32": 4}
    count = {k: (CHUNK if k == "observe_i32_65536" else M) for k in ops}
    v._stream()
    assert v._bound_stream == w._bound_stream
    stream = torch.cuda.current_stream(dev)
    times = {k: [] for k in ops}

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
    w.core.sync()
    # the paths agree: int32 planes in every byte, the puzzle, the position, and the other types' values
    ops["observe_i32"]()
    ch_loc = torch.stack([ch_pos & 0xFF, (ch_pos >> 8) & 0xFF], dim=1)
    equal = (bool(torch.equal(planes["i32"], ch_planes)) and bool(torch.equal(pidx, ch_pidx)) and
             bool(torch.equal(loc, ch_loc)))
    types_equal = True
    for c in range(0, M, CHUNK):                                     # (chunked: the int32 copies are large)
        s = slice(c, c + CHUNK)
        types_equal = types_equal and bool(torch.equal(planes["u8"][:, s].to(torch.int32), planes["i32"][:, s]))
        types_equal = types_equal and bool(torch.equal(net[s, cv].to(torch.int32), planes["i32"][0, s]))
        types_equal = types_equal and bool(torch.equal(net[s, ca].to(torch.int32), planes["i32"][1, s]))
    untouched = not bool(net[:, [0, 2, 4, 5, 6, 7]].any())
    row = {"records": M, "chunks_of_65536": M // CHUNK, "record_bytes": rb, "x_dim": X, "y_dim": Y, "rounds": a.calls,
           "planes_puzzle_position_equal_chained": equal, "other_types_equal_int32": types_equal,
           "other_channels_untouched": untouched, "fill_gbs": a.fill_gbs or None, "c4_obsw_gbs": C4_OBSW_GBS}
    for k in ops:
        t, n, eb = times[k], count[k], elem_bytes[k]
        med = float(np.median(t))
        written = n * (2 * XY * eb + 13) if k != "chained_i32" else n * (2 * XY * 4 + 8)
        read = n * (16 + 8 * table.words + (4 if tb else 0)) if k != "chained_i32" else None
        gbs = (written + (read or 0)) / med * 1e-3
        row[k] = {"median_us": round(med, 2), "p10_us": round(float(np.percentile(t, 10)), 2),
                  "p90_us": round(float(np.percentile(t, 90)), 2), "records": n, "bytes_written": written,
                  "bytes_read": read, "gb_per_s": round(gbs, 1),
                  "of_fill": round(gbs / a.fill_gbs, 4) if a.fill_gbs else None,
                  "launches": 1 if k != "chained_i32" else 4 * (M // CHUNK)}
    row["i32_p90_below_chained_p10"] = row["observe_i32"]["p90_us"] < row["chained_i32"]["p10_us"]
    row["i32_vs_chained"] = round(row["observe_i32"]["median_us"] / row["chained_i32"]["median_us"], 4)
    row["device"] = torch.cuda.get_device_name(0)
    v.close()
    w.close()
    print("ROW " + json.dumps(row), flush=True)


def readme(row, device):
    def line(k, what):
        r = row[k]
        fill = "not measured" if r["of_fill"] is None else f"{r['of_fill']:.3f}"
        return (f"| {what} | {r['records']:,} | {r['median_us']:,.2f} µs | {r['p10_us']:,.2f} .. {r['p90_us']:,.2f} | "
                f"{r['bytes_written']:,} | {r['gb_per_s']:,.1f} GB/s | {fill} | {r['gb_per_s'] / row['c4_obsw_gbs']:.3f} |")

    fill = "not measured in this job" if not row["fill_gbs"] else f"{row['fill_gbs']:,.1f} GB/s"
    return "\n".join([
        "# profiles/observe — observation planes of state records", "",
        f"- `prof_observe.json`: `python tools/prof_observe.py` on one MI355X (torch names it \"{device}\"). Device events around one path,",
        f"  median of {row['rounds']} rounds after {WARM} warm-up rounds, the paths alternating in one process. Workload: the c3",
        "  pool (1,024 puzzles, 7×7, traceback, `max_steps` 2000); the records are the `states` of the",
        "  `profiles/replay/` workload (65,536 sequences × 64 steps), the zeroed ones dropped with",
        f"  `Snapshot.select`, cut to {row['chunks_of_65536']} chunks of 65,536: {row['records']:,} records of {row['record_bytes']} B, planes {row['x_dim']}×{row['y_dim']}.",
        "- The chained path is what the parent commit offers from records to planes: per chunk",
        "  `sparc_restore_device` into a 65,536-env context, `sparc_obs_pack_device`, two",
        "  `sparc_copy_state_device`. It is int32 only: that path can produce no other element type, no",
        "  legal actions and no stride.",
        f"- Fill bandwidth (`tools/stream_bw`, nontemporal 16-B stores, same job): {fill}. `k_rollout_obsw` on c4:",
        f"  {row['c4_obsw_gbs']:,.1f} GB/s (`profiles/r06/final_bench/bench_c4.log`).", "",
        "| path | records | median | p10 .. p90 | bytes written | read + written / time | of fill | of c4 `k_rollout_obsw` |",
        "|---|---|---|---|---|---|---|---|",
        line("observe_i32", "`observe`, int32 dense"), line("observe_u8", "`observe`, uint8 dense"),
        line("observe_f16_2_of_8_channels", "`observe`, float16 into channels (3, 1) of 8"),
        line("observe_i32_65536", "`observe`, int32 dense, one chunk"),
        line("chained_i32", f"chained, int32: {row['chained_i32']['launches']} launches"), "",
        f"- Acceptance (int32 dense p90 below the chained path's p10): {row['i32_p90_below_chained_p10']}; "
        f"median ratio {row['i32_vs_chained']}.",
        f"- The int32 planes, the puzzle index and the position equal the chained path's in every byte: "
        f"{row['planes_puzzle_position_equal_chained']}; the uint8 and float16 planes equal them in value: "
        f"{row['other_types_equal_int32']}; the six other channels of the float16 tensor are untouched: "
        f"{row['other_channels_untouched']}.",
        "- Shapes behind the rows. Dense planes of a wave's 64 records are one run, written as whole 16-B pieces",
        "  whatever the plane size (the LUT path: 3 LDS reads per cell, so 12, 24 and 48 per piece of int32, float16",
        "  and uint8). A float16 plane of 49 cells is 98 B and the channels of an [M, 8, 7, 7] tensor start 98 B",
        "  apart, so the strided row's planes start off a 16-B boundary: each is 5 or 6 whole aligned pieces plus",
        "  element stores of up to 7 cells at either end, and it writes 2 of 8 channels, a quarter of every 784-B",
        "  row of the tensor. The one-chunk row is 65,536 records on 256 workgroups, one wave per SIMD, with the",
        "  launch and the tail in its time.", ""])


if a.worker:
    worker()
    sys.exit(0)

cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", "--calls", str(a.calls),
       "--puzzles", str(a.puzzles), "--roots", str(a.roots), "--per-root", str(a.per_root), "--horizon", str(a.horizon),
       "--fill-gbs", str(a.fill_gbs)]
p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
line = next((ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")), None)
if p.returncode != 0 or line is None:
    sys.exit(f"the GPU step ended with status {p.returncode}; nothing more is run")
row = json.loads(line[4:])
for k in ("observe_i32", "observe_u8", "observe_f16_2_of_8_channels", "observe_i32_65536", "chained_i32"):
    print(f"{k}: {row[k]['median_us']:.2f} us ({row[k]['p10_us']:.2f} .. {row[k]['p90_us']:.2f}), {row[k]['gb_per_s']:.1f} GB/s",
          flush=True)
print(f"records {row['records']}  i32/chained {row['i32_vs_chained']}  accepted {row['i32_p90_below_chained_p10']}  equal "
      f"{row['planes_puzzle_position_equal_chained']} {row['other_types_equal_int32']} {row['other_channels_untouched']}", flush=True)
device = row.pop("device")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump({"device": device, "timing": "device events around one path, median; the paths alternate in rounds "
               f"after {WARM} warm-up rounds", "chained": "per chunk of 65,536 records: sparc_restore_device into a "
               "65,536-env context, sparc_obs_pack_device, two sparc_copy_state_device (int32 only)", "rows": [row]},
              f, indent=1)
# the README's table is rewritten; what a person wrote below "## Reading" stays
path = os.path.join(os.path.dirname(os.path.abspath(a.out)), "README.md")
kept = open(path).read() if os.path.exists(path) else ""
kept = kept[kept.index("\n## Reading"):] if "\n## Reading" in kept else ""
with open(path, "w") as f:
    f.write(readme(row, device) + kept)
print("wrote", a.out)
if not (row["planes_puzzle_position_equal_chained"] and row["other_types_equal_int32"] and row["other_channels_untouched"]):
    sys.exit("the paths' outputs differ")
