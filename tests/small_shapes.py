"""Small batches and short launches for every rollout kernel family: which kernel a launch runs and
what it sees of it (families), the launch lengths and env counts that walk a tile pipeline's
prologue and epilogue and a grid's partial workgroups (launch_lengths, env_counts), the cases of
tests/test_gpu_small_shapes.py and the oracle's trace of each.  CPU helper: no GPU import.

Every rollout kernel is a software pipeline over tiles of L steps (L = 16, or RT in k_rollout1r) and
splits the batch into workgroups of E envs.  Which of its branches run depends on the number of
tiles in a launch, on a short last tile, and on whether the last workgroup is whole, so a case is
one context stepped through launch_lengths(L) back to back (the state crosses HBM at every launch
boundary, t0 is the running step count) at every env count of env_counts(E).

The oracle steps every env on its own: env i's puzzle, given actions and drawn actions
(counter hash of env_offset + i) do not depend on the batch size.  So the trace of a case is
computed once, at its largest env count, and a batch of n envs is compared with its first n columns.
The floors of what a trace must hold (assert_floors) are asserted on the oracle's trace alone."""
import collections
import functools
import zlib

import numpy as np

import rules_trace as rt
from oracle import COracle, OraclePool, RulesCOracle

KTILE = 16
ENV_OFFSET = 12345
# sparc_kernels.hip, rollout_impl: r1r_shape -> R1Shape<G, A, RT>; a workgroup holds 64 * G envs
R1R_SHAPES = {0: (2, 5, 15), 1: (4, 3, 12), 2: (2, 4, 12), 3: (4, 1, 4), 4: (2, 3, 15), 5: (2, 5, 10)}


# ----------------------------------------------------------------------------- dispatch, restated
def base_families(table, n, T):
    """The kernels one sparc_rollout_device call of T steps runs on n envs with 16-B aligned
    buffers: the dispatch conditions of rollout_impl (sparc_kernels.hip), restated."""
    tiled = n % 16 == 0
    if table.words == 1:
        # split1_pitch_ok and the 8-B trie records (every trie below 2^15 nodes)
        split = tiled and n % 256 == 0 and T >= 16 and 3 <= table.pitch <= 9 and int(table.info[:, 3].max()) <= 0x7FFF
        generic = "k_rollout1"
    else:
        # split_w of build_puzzle_tables: pitch <= 15, small tries, and the LDS layout fits, which
        # tests/test_tables_host.py asserts for the gap-free 9x9 and 15x15 tables
        split = (tiled and n % 256 == 0 and T >= 16 and table.pitch <= 15
                 and int(table.info[:, 3].max()) <= 0x7FFF)
        generic = "k_rollout"
    if not split:
        return {generic}
    return {"k_rollout1s" if table.words == 1 else "k_rolloutWs"} | ({generic} if T % 16 else set())


def families(table, n, T, *, given=True, obs=False, rules=False, variant=None, tab_all=True):
    """The kernels one rollout call of T steps runs on n envs (16-B aligned buffers), in launch
    order, each as a dict: kernel, its tile length L and workgroup size E, the steps it runs, the
    full tiles and the short last tile it sees (the split kernels hand T % 16 steps over to
    k_rollout1 / k_rollout), whether its I/O is tiled, whether its last workgroup is full, and
    `piped`: whether any of its workgroups (waves, in the generic kernel) runs the tiled pipeline
    and not the per-step byte paths.  variant: {"IO_CODES_OFF" | "RULE_ROLLOUT_GENERIC" |
    "R1R_SHAPE" | "OBS_INLINE": value} as sparc_set_variant; tab_all: every puzzle of a one-word
    rule pool has its region-code table."""
    variant = variant or {}
    tiled = n % 16 == 0

    def part(kernel, steps, L=KTILE, E=256, unit=None, tiles=True, **kw):
        unit = unit or E                                  # the envs that take the tiled path together
        piped = tiles and tiled and n >= unit
        # k_rollout1 and the generic kernel have a tile loop on the tiled path only: elsewhere every
        # step is a "tail" step; the other kernels step tile by tile whatever the batch
        tile_loop = piped or kernel not in ("k_rollout1", "k_rollout", "k_rollout_obs", "k_rollout_rules")
        full = steps // L if tile_loop else 0
        return dict(kernel=kernel, L=L, E=E, steps=steps, full_tiles=full, short=steps - full * L, tiled=tiled,
                    last_wg_full=n % E == 0, piped=piped, workgroups=-(-n // E), **kw)

    if rules:
        ring_ok = table.words == 1 and all(int(x) * table.pitch <= 57 for x in table.info[:, 0] & 0xFF)
        if table.words == 1 and tab_all and ring_ok and not variant.get("RULE_ROLLOUT_GENERIC"):
            G, A, RT = R1R_SHAPES[variant.get("R1R_SHAPE", 0)]
            return [part("k_rollout1r", T, L=RT, E=64 * G, shape=(G, A, RT))]
        return [part("k_rollout_rules", T, E=128, unit=64)]       # k_rollout<..., RULES>: wave pairs of 64 envs
    if obs:
        if variant.get("OBS_INLINE"):
            return [part("k_rollout_obs", T, unit=64)]            # k_rollout<..., OBS>
        # one barrier per step, two staging buffers: a "tile" of the writer-wave kernel is 2 steps
        return [part("k_rollout_obsw", T, L=2, tiles=False)]
    out = []
    names = base_families(table, n, T)
    split = names & {"k_rollout1s", "k_rolloutWs"}
    if split:
        kernel = split.pop()
        pr = 1 if (kernel == "k_rollout1s" and given and n // 256 <= 64) else 4
        ior = not variant.get("IO_CODES_OFF")                     # and next-step autoreset (the caller's)
        out.append(part(kernel, T // KTILE * KTILE, E=64 * pr if kernel == "k_rollout1s" else 256, PR=pr, IOR=ior))
        T -= T // KTILE * KTILE
    if T:
        generic = (names - {"k_rollout1s", "k_rolloutWs"}).pop()
        out.append(part(generic, T, unit=256 if generic == "k_rollout1" else 64))
    return out


def shape_class(n, E):
    """What a grid of n envs in workgroups of E is, in the classes the guard test asks for."""
    if n < 64:
        return "below_a_wave"
    if n == 64:
        return "one_wave"
    if n < E:
        return "partial_workgroup"
    return {E: "full_workgroup", E + 1: "full_plus_1", E + 16: "full_plus_16"}.get(n, "more")


# ----------------------------------------------------------------------------- the shape lists
def launch_lengths(L, kernel=None, ior=False):
    """The steps of the launches of one case, run back to back, for a kernel with tiles of L steps:
    0 to 5 full tiles, each with and without a short last tile, and what the kernel's buffers add."""
    Ts = [1, 2, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 3 * L, 3 * L + 1, 4 * L, 4 * L + 1, 5 * L, 5 * L + 3]
    if kernel in ("k_rollout1", "k_rollout1s", "k_rolloutWs"):
        # the output rings hold 4 tiles (kRing = 64 rows): with 6 tiles the epilogue stores tiles
        # K-2 and K-1 from ring slots 0 and 1, both written a second time (k_rollout1s's three
        # action buffers have then gone round twice)
        Ts.append(6 * L)
        # 8 tiles and a tail: ring slot 0 is written a third time, the stores of the loop body
        # (tile k-2 in interval k) wrap once more
        Ts.append(8 * L + 9)
    if kernel in ("k_rollout1s", "k_rolloutWs") and ior:
        # IOR: the I/O waves flush their byte counters after tile 127 (flush_counts / io_flush at
        # (k - 2) & 127 == 127) and again at the end: one launch past that flush
        Ts.append(130 * L + 5)
    if kernel == "k_rollout1r":
        # three reward / flag buffers (tile % 3) and two ring / rule-bit buffers (tile & 1): after 6
        # full tiles both have come round together, 6 L + 1 starts the next turn with a 1-step tile
        Ts += [6 * L, 6 * L + 1]
    if kernel == "k_rollout_obsw":
        # L = 2 (the two staging buffers): a launch long enough that the writers run many steps behind
        # one barrier each, odd so that the last step leaves through buffer 0
        Ts.append(33)
    return tuple(dict.fromkeys(t for t in Ts if t > 0))


def env_counts(E):
    """The env counts for a kernel whose workgroup holds E envs."""
    return tuple(sorted({1, 2, 3, 15, 16, 17, 48, 63, 64, 65, 80, E - 16, E - 1, E, E + 1, E + 16, 2 * E}))


def trimmed_counts(E):
    """The shorter list for pool D, the OBS_INLINE variant and k_rollout1r shapes 1-5."""
    return tuple(sorted({1, 17, 63, 64, 65, E - 1, E, E + 1, E + 16}))


# the split kernels run whole 256-env workgroups only; 240 (tiled) and 257 (untiled) fall to the
# fallback kernel of the same pool
SPLIT_COUNTS = (240, 256, 257, 512)


# ----------------------------------------------------------------------------- pools
# make_puzzles pools as tests/test_gpu_parity.POOLS (which test_gpu_small_shapes.py asserts)
STEP_SIZES = {"7x7_full": ((3, 3),), "mixed_5_11": ((2, 2), (3, 3), (4, 4), (5, 5), (2, 5), (5, 3)),
              "15x15": ((7, 7), (6, 7))}
N_PUZZLES = 64
Pool = collections.namedtuple("Pool", "proc table opool rules p0 allpass")


@functools.lru_cache(maxsize=None)
def pool(name):
    """Pool `name`: at most 64 processed puzzles, their table, the OraclePool, the RulesCOracle of a
    rule pool, and p0, the puzzle env 0 starts on: the one with the shortest listed solution (so
    that env 0 solves it within max_steps), among those whose solution passes every rule where a rule
    pool has one (allpass).  Built once per process; read only."""
    from sparc_gym_amd import synthetic
    from sparc_gym_amd.puzzles import pack_table, process_puzzles
    rules = None
    if name in STEP_SIZES:
        proc = process_puzzles(synthetic.make_puzzles(N_PUZZLES, seed=len(name), sizes=STEP_SIZES[name],
                                                      full_properties=True))
        table = pack_table(proc)
    elif name in rt.POOLS:
        full = rt.pool(name)[0]                  # 128 rule-consistent + 128 random: 32 of each
        proc = full[:N_PUZZLES // 2] + full[128:128 + N_PUZZLES // 2]
        table = pack_table(proc)
        rules = RulesCOracle(proc)
    else:
        import geometry_pools as gp
        proc, table, _ = gp.step_pool(name)
    assert len(proc) <= N_PUZZLES
    lens = np.array([len(p["solution_paths"][0]) if len(p["solution_paths"]) else 1 << 20 for p in proc])
    allpass = []
    if rules is not None:
        for q, p in enumerate(proc):
            if len(p["solution_paths"]):
                s = [list(map(int, pt)) for pt in p["solution_paths"][0]]
                if rules.bits(q, s, s[-1]) >> 8 & 1:
                    allpass.append(q)
    cand = allpass or range(len(proc))
    p0 = min(cand, key=lambda q: (lens[q], q))
    return Pool(proc, table, OraclePool(rt.step_pool(proc)), rules, int(p0), bool(allpass))


def puzzle_indices(name, n):
    P = pool(name)
    return (P.p0 + np.arange(n) * 37) % len(P.proc)


# ----------------------------------------------------------------------------- cases
def _case(kernel, pool_name, tb, autoreset, given=True, *, L=KTILE, E=256, ns=None, obs=False, rules=False,
          variant=(), max_steps=16, tag=None):
    variant = dict(variant)
    ior = kernel in ("k_rollout1s", "k_rolloutWs") and autoreset == "next_step" and not variant.get("IO_CODES_OFF")
    cid = "-".join([kernel, pool_name, f"tb{int(tb)}", autoreset, "given" if given else "drawn"]
                   + [f"{k}={v}" for k, v in variant.items()] + ([tag] if tag else []))
    return dict(id=cid, kernel=kernel, pool=pool_name, tb=tb, autoreset=autoreset, given=given, L=L, E=E,
                ns=tuple(ns if ns is not None else env_counts(E)), obs=obs, rules=rules, variant=variant,
                max_steps=max_steps, Ts=launch_lengths(L, kernel, ior), seed=SEEDS.get(cid, 1))


# The first action seed in 1, 2, 3, ... with which the ORACLE's trace of the case meets assert_floors on
# env 0 alone (find_seed; no GPU output feeds it); a case not listed meets them with seed 1.
SEEDS = {
    "k_rollout1-7x7_full-tb0-next_step-given": 3,
    "k_rollout1-7x7_full-tb1-next_step-given": 2,
    "k_rollout1-7x7_full-tb1-next_step-drawn": 4,
    "k_rollout1-w1p10-tb0-next_step-given": 2,
    "k_rollout1-w1p10-tb1-next_step-given": 2,
    "k_rollout1s-7x7_full-tb1-next_step-given": 2,
    "k_rollout1s-7x7_full-tb0-next_step-drawn": 4,
    "k_rollout1s-7x7_full-tb1-next_step-drawn": 4,
    "k_rollout1s-7x7_full-tb1-next_step-drawn-IO_CODES_OFF=1": 4,
    "k_rollout1s-7x7_full-tb1-next_step-given-IO_CODES_OFF=1": 2,
    "k_rolloutWs-mixed_5_11-tb1-next_step-drawn": 3,
    "k_rollout-mixed_5_11-tb1-next_step-given": 2,
    "k_rollout-mixed_5_11-tb0-next_step-drawn": 5,
    "k_rolloutWs-15x15-tb0-next_step-given": 3,
    "k_rolloutWs-15x15-tb1-next_step-given": 8,
    "k_rolloutWs-15x15-tb1-next_step-drawn": 2,
    "k_rollout-15x15-tb0-next_step-given": 5,
    "k_rollout-15x15-tb1-next_step-given": 91,
    "k_rollout_obsw-7x7_full-tb1-next_step-drawn": 2,
    "k_rollout_obsw-mixed_5_11-tb1-next_step-drawn": 3,
    "k_rollout_obsw-15x15-tb1-next_step-drawn": 2,
    "k_rollout_obs-15x15-tb0-next_step-given-OBS_INLINE=1": 2,
    "k_rollout_obs-15x15-tb1-next_step-given-OBS_INLINE=1": 11,
    "k_rollout_obs-7x7_full-tb0-next_step-drawn-OBS_INLINE=1": 4,
    "k_rollout1r-A-tb0-next_step-drawn": 8,
    "k_rollout1r-B-tb0-next_step-given": 2,
    "k_rollout1r-B-tb1-next_step-given": 2,
    "k_rollout1r-A-tb0-next_step-given-R1R_SHAPE=1": 4,
    "k_rollout1r-A-tb1-next_step-given-R1R_SHAPE=2": 3,
    "k_rollout1r-A-tb0-next_step-given-R1R_SHAPE=3": 2,
    "k_rollout_rules-A-tb0-next_step-given-RULE_ROLLOUT_GENERIC=1": 4,
    "k_rollout_rules-A-tb1-next_step-drawn-RULE_ROLLOUT_GENERIC=1": 4,
    "k_rollout_rules-C-tb1-next_step-given": 2,
    "k_rollout_rules-D-tb0-next_step-given": 2,
}


def _build_cases():
    both, modes = (False, True), ("next_step", "none")
    not256 = [n for n in env_counts(256) if n % 256]
    c = []
    # k_rollout1: the 7x7 pool away from whole 256-env batches, and a one-word pool of pitch 10
    # (outside split1_pitch_ok's 3..9) at whole ones
    c += [_case("k_rollout1", "7x7_full", tb, ar, ns=not256) for tb in both for ar in modes]
    c += [_case("k_rollout1", "7x7_full", True, "next_step", False, ns=not256)]
    c += [_case("k_rollout1", "w1p10", tb, ar, ns=(256, 512)) for tb in both for ar in modes]
    # k_rollout1s and its k_rollout1 tail: given actions run <PR = 1> (look-ahead), drawn ones <PR = 4>
    c += [_case("k_rollout1s", "7x7_full", tb, ar, ns=SPLIT_COUNTS) for tb in both for ar in modes]
    c += [_case("k_rollout1s", "7x7_full", tb, "next_step", False, ns=SPLIT_COUNTS) for tb in both]
    c += [_case("k_rollout1s", "7x7_full", True, "next_step", given, ns=SPLIT_COUNTS, variant={"IO_CODES_OFF": 1})
          for given in both]
    # k_rolloutWs and its k_rollout tail; the generic k_rollout at the other env counts
    for name, ms, ars in (("mixed_5_11", 16, modes), ("15x15", 24, ("next_step",))):
        c += [_case("k_rolloutWs", name, tb, ar, ns=SPLIT_COUNTS, max_steps=ms) for tb in both for ar in ars]
        c += [_case("k_rolloutWs", name, True, "next_step", False, ns=SPLIT_COUNTS, max_steps=ms)]
        c += [_case("k_rollout", name, tb, "next_step", ns=not256, max_steps=ms) for tb in both]
        c += [_case("k_rollout", name, False, "next_step", False, ns=not256, max_steps=ms)]
    # the observation rollouts: writer waves (two staging buffers: L = 2) and the inline variant
    for name, ms in (("7x7_full", 16), ("mixed_5_11", 16), ("15x15", 24)):
        # (their launches are short: max_steps 12, so that episodes end inside them)
        c += [_case("k_rollout_obsw", name, tb, "next_step", L=2, obs=True, max_steps=12) for tb in both]
        c += [_case("k_rollout_obsw", name, True, "next_step", False, L=2, obs=True, max_steps=12)]
        c += [_case("k_rollout_obs", name, tb, "next_step", obs=True, ns=trimmed_counts(256), max_steps=ms,
                    variant={"OBS_INLINE": 1}) for tb in both]
    c += [_case("k_rollout_obs", "7x7_full", False, "next_step", False, obs=True, ns=trimmed_counts(256),
                variant={"OBS_INLINE": 1})]
    # k_rollout1r: shape 0 in full (pools A and B), shapes 1-5 on the trimmed list
    G, A, RT = R1R_SHAPES[0]
    c += [_case("k_rollout1r", "A", tb, ar, L=RT, E=64 * G, rules=True) for tb in both for ar in modes]
    c += [_case("k_rollout1r", "A", False, "next_step", False, L=RT, E=64 * G, rules=True)]
    c += [_case("k_rollout1r", "B", tb, "next_step", L=RT, E=64 * G, rules=True) for tb in both]
    for s in (1, 2, 3, 4, 5):
        G, A, RT = R1R_SHAPES[s]
        c += [_case("k_rollout1r", "A", s % 2 == 0, "next_step", s != 5, L=RT, E=64 * G, rules=True,
                    ns=trimmed_counts(64 * G), variant={"R1R_SHAPE": s})]
    # the generic rule kernel (wave pairs: 128 envs per workgroup)
    c += [_case("k_rollout_rules", "A", tb, "next_step", E=128, rules=True, variant={"RULE_ROLLOUT_GENERIC": 1})
          for tb in both]
    c += [_case("k_rollout_rules", "A", True, "next_step", False, E=128, rules=True,
                variant={"RULE_ROLLOUT_GENERIC": 1})]
    c += [_case("k_rollout_rules", "C", True, "next_step", E=128, rules=True, max_steps=24)]
    c += [_case("k_rollout_rules", "D", False, "next_step", E=128, rules=True, ns=trimmed_counts(128), max_steps=24)]
    return c


CASES = _build_cases()
CASE = {c["id"]: c for c in CASES}
assert len(CASE) == len(CASES)
PARAMS = [(c["id"], n) for c in CASES for n in c["ns"]]


# ----------------------------------------------------------------------------- the oracle's side
def given_actions(c, n, T):
    """[T, n] uint8: rules_trace.actions (even envs start along a listed solution of their puzzle,
    then uniform 0..4), with every other 4 turned into 255: both are "no such action"."""
    P = pool(c["pool"])
    assert n <= N_ACTION_ENVS
    # drawn at one width whatever n, so that env i's actions do not depend on the batch size
    a = rt.actions(P.proc, puzzle_indices(c["pool"], N_ACTION_ENVS), T,
                   c["seed"] + zlib.crc32(c["id"].encode()) % 1000)[:, :n].copy()
    t, i = np.indices(a.shape)
    a[(a == 4) & ((t + i) % 2 == 1)] = 255
    assert (a == 4).any() and (a == 255).any()
    return a


N_ACTION_ENVS = 576
Trace = collections.namedtuple("Trace", "acts launches state legal0 n")


def _trace(c, n):
    P = pool(c["pool"])
    Ts = c["Ts"]
    o = COracle(P.opool, n, c["tb"], c["max_steps"], autoreset={"none": 0, "next_step": 1}[c["autoreset"]])
    o.reset(puzzle_indices(c["pool"], n))
    legal0 = np.array([o.legal(i) for i in range(min(n, 4))], np.uint8)
    acts = given_actions(c, n, sum(Ts)) if c["given"] else None
    stats = np.zeros((n, 4), np.int32)
    launches, t0 = [], 0
    for T in Ts:
        a = None if acts is None else acts[t0:t0 + T]
        kw = dict(seed=c["seed"], env_offset=0 if c["given"] else ENV_OFFSET, t0=t0, stats=stats)
        if c["rules"]:
            rew, flags, bits = o.rollout_rules(T, P.rules, a, **kw)
        else:
            (rew, flags), bits = o.rollout(T, a, **kw), None
        launches.append(dict(t0=t0, T=T, rew=rew, flags=flags, bits=bits, stats=stats.copy()))
        t0 += T
    if acts is None:   # the drawn actions of the first envs, for the illegal-action floor
        acts = np.array([[o.rand_action(c["seed"], ENV_OFFSET + i, t) for i in range(min(n, 4))]
                         for t in range(sum(Ts))], np.uint8)
    state = o.state()
    for v in [acts, *state.values()] + [x for l in launches for x in l.values() if isinstance(x, np.ndarray)]:
        v.setflags(write=False)
    return Trace(acts, launches, state, legal0, n)


@functools.lru_cache(maxsize=None)
def trace(cid):
    """The oracle's trace of case `cid` at its largest env count, launch by launch: a batch of n
    envs is its first n columns.  Computed once per process; read only."""
    c = CASE[cid]
    return _trace(c, max(c["ns"]))


def floors(c, tr, n):
    """What the first n envs of the oracle's trace `tr` of case c hold: a dict of counts."""
    flags = np.concatenate([l["flags"][:, :n] for l in tr.launches])
    T = len(flags)
    ends = np.cumsum([l["T"] for l in tr.launches])              # steps after each launch
    done = (flags & 3) != 0
    m = min(n, tr.acts.shape[1], len(tr.legal0))
    legal = np.vstack([tr.legal0[None, :m], (flags[:-1, :m] >> 2) & 0xF])   # the legal set each step acts on
    a = tr.acts[:T, :m]
    live = (flags[:, :m] & 64) == 0        # an autoreset step takes no action (without autoreset the steps
    #                                         past an episode's end still run the whole step)
    out = dict(terminated=int((flags & 1).astype(bool).sum()), truncated=int((flags & 2).astype(bool).sum()),
               illegal=int((live & ((a >= 4) | (((legal >> np.minimum(a, 3)) & 1) == 0))).sum()),
               autoresets=int(((flags & 64) != 0).sum()),
               autoreset_first=int(((flags[ends[:-1]] & 64) != 0).sum()),   # ... as a launch's first step
               done_last=int(done[ends - 1].sum()))                         # a done step as a launch's last
    if c["rules"]:
        bits = np.concatenate([l["bits"][:, :n] for l in tr.launches])
        out.update(patterns=len(np.unique(bits)), allpass=int(((bits >> 8) & 1).sum()), minus1=int((bits == -1).sum()))
    return out


def assert_floors(c, tr, n):
    f = floors(c, tr, n)
    assert f["terminated"] >= 1 and f["truncated"] >= 1 and f["illegal"] >= 1, (c["id"], n, f)
    if c["autoreset"] == "next_step":
        assert f["autoresets"] >= 1 and f["autoreset_first"] >= 1 and f["done_last"] >= 1, (c["id"], n, f)
    if c["rules"]:
        assert f["minus1"] == 0 and f["patterns"] >= 2, (c["id"], n, f)
        if pool(c["pool"]).allpass:
            assert f["allpass"] >= 1, (c["id"], n, f)
    return f


def find_seed(cid, limit=400):
    """The first seed with which env 0 alone meets the floors (then so does every env count)."""
    for seed in range(1, limit):
        c = dict(CASE[cid], seed=seed)
        try:
            assert_floors(c, _trace(c, 4), 1)
        except AssertionError:
            continue
        return seed
    raise LookupError(cid)
