"""Tree search helpers on top of ``SPaRCVecEnv.expand``: a frontier of positions is a ``Snapshot``
(one record per node, any number of them), and one level of a search is one ``expand`` launch
plus a compaction of the children worth keeping.

The rule the helpers follow is the reference's own: a state that is done (terminated or
truncated, step(), SPaRC_Gym.py:1192-1199) has no successors, and the successors of a live state
are its legal actions (_get_legal_actions, 1024-1051).  Illegal actions, which ``expand`` also
steps (the no-move state with step + 1), are dropped here.

The compaction is plain torch indexing on the GPU (``nonzero`` + a row gather); its order is the
ascending child index, parent-major then action, so every result is deterministic.  Not done
here: detecting the same position reached twice within a frontier, and compaction inside the
kernel.

``solve_dfs`` needs neither a frontier per level nor a compaction: after a few split levels it
hands every node to ``SPaRCVecEnv.dfs``, which walks the subtree below it depth-first on the GPU
(the record's direction stack is the search stack) and returns counters, so its memory does not
depend on the tree.
"""
from __future__ import annotations

import numpy as np
import torch

from .rules import RULE_ALL

DONE_BITS = 3   # flags bit 0 terminated, bit 1 truncated
TERMINATED = 1  # flags bit 0: the agent is on the target (step(), SPaRC_Gym.py:1192)


def _done_mask(done, M, device):
    """[M] bool from a bool mask, 0/1 bytes or step flags (bits 0-1)."""
    d = torch.as_tensor(np.asarray(done) if not isinstance(done, torch.Tensor) else done, device=device)
    if d.shape != (M,):
        raise ValueError(f"done must have shape ({M},)")
    if d.dtype == torch.bool:
        return d
    if d.dtype.is_floating_point:
        raise ValueError("done must be a bool mask or flag bytes")
    return (d.to(torch.int64) & DONE_BITS) != 0


def expand_frontier(vec, snap, done=None, prune=False):
    """Expand ``snap`` once and keep only the children that are real moves of a live parent:
    child ``(j, a)`` stays iff bit ``a`` of parent ``j``'s legal mask is set and ``done[j]`` is
    not.  ``done``: [M] bool, or the flag bytes the parents were produced with (bits 0-1:
    terminated, truncated); default: every parent is live.  Returns a dict: ``children`` (a
    ``Snapshot`` of the K kept records, on the GPU), ``parent`` [K] int64 (row of ``snap``),
    ``action`` [K] int64, ``reward_code`` [K] int8, ``flags`` [K] uint8, in ascending
    ``4 * parent + action``.  ``flags`` are the done bits for the next level.

    ``prune=True``: child ``(j, a)`` stays only if bit ``a`` of ``vec.reach(snap)["live"]`` is also
    set, that is, if the target can still be reached from it over the points the path has left
    free.  A child that cannot is lost with everything below it; the children that are traceback
    pops go as well (they lead onto a visited point).  The order of the kept rows is unchanged."""
    out = vec.expand(snap)
    M = len(snap)
    legal = out["legal_mask"].to(torch.int64)
    if prune:
        legal = legal & vec.reach(snap)["live"].to(torch.int64)
    keep = ((legal[:, None] >> torch.arange(4, device=legal.device)) & 1) != 0
    if done is not None:
        keep &= ~_done_mask(done, M, legal.device)[:, None]
    idx = keep.reshape(-1).nonzero().squeeze(1)          # ascending child index
    return {"children": out["children"].select(idx), "parent": idx >> 2, "action": idx & 3,
            "reward_code": out["reward_code"].reshape(-1)[idx], "flags": out["flags"].reshape(-1)[idx]}


def enumerate_paths(vec, puzzle_indices, max_depth=None, max_frontier=1 << 22):
    """Level-synchronous breadth-first expansion of the legal-move trees of ``puzzle_indices``
    (one root per entry: that puzzle's reset state), all roots at once.  A node is expanded iff
    it is not done; its children are its legal actions.  Stops after ``max_depth`` levels or when
    no live node is left, and raises RuntimeError if a level holds more than ``max_frontier``
    nodes.  With traceback every move can be undone, so the tree ends only through
    ``max_steps``: give ``max_depth``.

    The roots come from ``vec.reset`` and ``vec.snapshot``, so ``vec`` needs at least
    ``len(puzzle_indices)`` envs and its state is overwritten.

    Returns a dict of int64 arrays [R, D + 1] (D: the deepest level reached; column 0 is the
    roots): ``nodes`` the nodes at each depth, ``solved`` those that ended with reward code +100,
    ``ended`` those that ended otherwise (terminated or truncated); and ``solution``: per root,
    the actions of one path to a +100 node (the shallowest, lowest-index one) or None."""
    q = np.asarray(puzzle_indices, np.int64)
    R = len(q)
    if q.ndim != 1 or R < 1 or R > vec.num_envs:
        raise ValueError(f"puzzle_indices must hold 1..{vec.num_envs} puzzle indices")
    full = np.full(vec.num_envs, q[0], np.int64)
    full[:R] = q
    vec.reset(options={"puzzle_index": full})
    frontier = vec.snapshot(envs=np.arange(R))
    dev = frontier.records.device
    root = torch.arange(R, device=dev)
    nodes, solved, ended = [np.ones(R, np.int64)], [np.zeros(R, np.int64)], [np.zeros(R, np.int64)]
    levels = []                                          # per level: parent, action, live rows
    found = {}                                           # root -> (level, row) of its first +100 node
    depth = 0
    while len(frontier) and (max_depth is None or depth < max_depth):
        out = expand_frontier(vec, frontier)             # the frontier holds live nodes only
        K = len(out["children"])
        if K == 0:                                       # roots without a legal move
            break
        if K > max_frontier:
            raise RuntimeError(f"depth {depth + 1} holds {K} nodes, more than max_frontier = {max_frontier}")
        depth += 1
        croot = root[out["parent"]]
        done = (out["flags"] & DONE_BITS) != 0
        win = out["reward_code"] == 100
        count = lambda m: torch.bincount(croot[m], minlength=R).cpu().numpy().astype(np.int64)  # noqa: E731
        nodes.append(torch.bincount(croot, minlength=R).cpu().numpy().astype(np.int64))
        solved.append(count(done & win))
        ended.append(count(done & ~win))
        rows = (done & win).nonzero().squeeze(1)
        if len(rows):
            rows_h = rows.cpu().numpy()
            for r, k in zip(*np.unique(croot[rows].cpu().numpy(), return_index=True)):
                found.setdefault(int(r), (depth, int(rows_h[k])))
        # the live nodes are the next frontier; a level keeps, for the walk back to the root, its
        # nodes' parent (a row of the frontier it was expanded from) and action, and the level
        # rows that became the next frontier
        live = (~done).nonzero().squeeze(1)
        levels.append((out["parent"].cpu().numpy(), out["action"].cpu().numpy(), live.cpu().numpy()))
        frontier = out["children"].select(live)
        root = croot[live]
    solution = [None] * R
    for r, (d, row) in found.items():
        acts = []
        while d >= 1:
            parent, action, _ = levels[d - 1]
            acts.append(int(action[row]))
            prow = int(parent[row])                      # a row of the frontier expanded at level d
            row = prow if d == 1 else int(levels[d - 2][2][prow])
            d -= 1
        solution[r] = acts[::-1]
    return {"nodes": np.stack(nodes, 1), "solved": np.stack(solved, 1), "ended": np.stack(ended, 1),
            "solution": solution}


def rand_pick(seed, id, t, mask):
    """``sparc_rand_pick`` (include/sparc_gym_amd.h) on numpy arrays, broadcast together: the
    uniform draw of ``SPaRCVecEnv.playout`` among the set bits of ``mask & 15``.  With ``z`` the
    splitmix64 finaliser of ``(seed, id, t)``, ``n = popcount(mask & 15)`` and
    ``r = ((z >> 32) * n) >> 32``, the index of the r-th set bit counted from bit 0; 0 for an
    empty mask.  uint64 arithmetic throughout; returns int64."""
    def u(v):   # a Python int is taken modulo 2^64, as the C argument is
        return np.uint64(v & (2**64 - 1)) if isinstance(v, int) else np.asarray(v).astype(np.uint64)

    seed, id, t, m = np.broadcast_arrays(u(seed), u(id), u(t), u(mask) & np.uint64(15))
    with np.errstate(over="ignore"):
        z = seed + id * np.uint64(0x9E3779B97F4A7C15) + t * np.uint64(0xD1B54A32D192ED03)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    bits = [(m >> np.uint64(d)) & np.uint64(1) for d in range(4)]
    n = bits[0] + bits[1] + bits[2] + bits[3]
    r = ((z >> np.uint64(32)) * n) >> np.uint64(32)          # < 2^34: no overflow
    out = np.zeros(m.shape, np.int64)
    seen = np.zeros(m.shape, np.uint64)
    for d in range(4):
        out = np.where((bits[d] == 1) & (seen == r), d, out)
        seen = seen + bits[d]
    return out


def monte_carlo(vec, snap, playouts, horizon, seed=0, forward_only=None):
    """Flat Monte-Carlo evaluation of every record of ``snap`` (M of them): one
    ``vec.playout(snap, playouts, horizon, ...)`` launch with the trace, reduced per record and
    first action.  ``forward_only`` defaults to ``vec.traceback`` (a uniform walk that may undo
    its moves rarely arrives).  Touches no env.

    Returns a dict: ``visits``, ``wins``, ``losses`` [M, 4] int64 (playouts that began with action
    a; those whose last reward code was +100 / -100) and ``mean_steps`` [M, 4] float64 (0 where
    no visit), as numpy arrays; ``best_action`` [M] int64: the action with the highest
    ``wins / visits`` among those visited (only legal actions are ever drawn; ties go to the
    lowest action), -1 where no playout took a step; ``solution``: per record, the action list
    of its shortest playout that ended with code +100 (the lowest k wins ties), or None."""
    if forward_only is None:
        forward_only = bool(vec.traceback)
    out = vec.playout(snap, playouts, horizon, seed=seed, forward_only=forward_only, trace=True, stats=True)
    stats = out["stats"].cpu().numpy().astype(np.int64)      # [M, 4, 4]
    visits, wins, losses, steps = (stats[:, :, c] for c in range(4))
    mean_steps = np.where(visits > 0, steps / np.maximum(visits, 1), 0.0)
    rate = np.where(visits > 0, wins / np.maximum(visits, 1), -1.0)
    best = np.where((visits > 0).any(1), rate.argmax(1), -1).astype(np.int64)   # argmax: the first maximum
    code = out["reward_code"].cpu().numpy()
    nsteps = out["steps"].cpu().numpy().astype(np.int64)
    trace = out["trace"].cpu().numpy()                       # [L, M, K]
    won = (code == 100) & (nsteps > 0)
    solution = [None] * len(visits)
    for j in np.nonzero(won.any(1))[0]:
        k = int(np.where(won[j], nsteps[j], np.iinfo(np.int64).max).argmin())   # the first minimum
        solution[j] = [int(a) for a in trace[:nsteps[j, k], j, k]]
    return {"visits": visits, "wins": wins, "losses": losses, "mean_steps": mean_steps, "best_action": best,
            "solution": solution}


def uct(vec, snap, sims, horizon, c=1.0, trees=1, explore=None, seed=0, forward_only=None, tree=None, cap=None):
    """UCT search of every record of ``snap`` (M of them) with ``vec.mcts``: ``sims`` simulations on
    each of ``trees`` independent trees per record in ONE launch.  Record ``j`` is repeated
    ``trees`` times (rows ``j * trees .. j * trees + trees - 1`` of the search), the rows are
    distinct and so are their random streams: root parallelism.  ``tree``: the ``tree`` of a previous
    call with the same ``snap`` and ``trees``, to continue it; ``cap``, ``c``, ``explore``, ``seed``
    and ``forward_only`` as ``vec.mcts``.  Touches no env.

    Returns a dict: ``visits``, ``wins``, ``losses`` [M, 4] int64 numpy arrays, the roots' per-action
    ``n``, ``wins`` and the children's own losses summed over the trees; ``best_action`` [M] int64,
    the most visited action (ties go to the lowest action), -1 where no action has a visit (a root
    that is done, walled in or refused); ``solution``: per record the action list, from the puzzle's
    start, of the shortest winning path its trees have found (the lowest tree wins ties), or None
    (always None without traceback: such records hold no moves); ``status`` [M, trees] and
    ``tree``: what ``vec.mcts`` returned for the ``M * trees`` rows."""
    from . import _lib
    M, trees = len(snap), int(trees)
    if M < 1 or trees < 1:
        raise ValueError("at least one record and one tree are needed")
    rows = torch.arange(M * trees) // trees
    out = vec.mcts(snap.select(rows), sims, horizon, c=c, explore=explore, tree=tree, cap=cap, seed=seed,
                   forward_only=forward_only)
    nodes = out["nodes"].view(torch.int32)                                     # [M * trees, cap, 16]
    root = nodes[:, 0].to(torch.int64) & 0xFFFFFFFF
    child = root[:, _lib.MCTS_CHILD:_lib.MCTS_CHILD + 4]
    real = (child != 0) & (child < nodes.shape[1])                             # (MCTS_NO_CHILD lies above every cap)
    own = torch.gather(nodes[:, :, _lib.MCTS_LOSSES], 1, torch.where(real, child, torch.zeros_like(child)))
    own = own.to(torch.int64) & 0xFFFFFFFF
    started = (out["count"] > 0)[:, None]                                      # an untouched arena holds no root

    def total(x):
        return torch.where(started, x, torch.zeros_like(x)).reshape(M, trees, 4).sum(1).cpu().numpy()

    visits = total(root[:, _lib.MCTS_N:_lib.MCTS_N + 4])
    wins = total(root[:, _lib.MCTS_CHILD_WINS:_lib.MCTS_CHILD_WINS + 4])
    losses = total(torch.where(real, own, torch.zeros_like(own)))
    best = np.where((visits > 0).any(1), visits.argmax(1), -1).astype(np.int64)   # argmax: the first maximum
    steps = out["win_steps"].reshape(M, trees).cpu().numpy()
    solution = [None] * M
    if vec.traceback:
        won = np.nonzero((steps >= 0).any(1))[0]
        k = np.where(steps >= 0, steps, np.iinfo(np.int64).max).argmin(1)         # the first minimum
        if len(won):
            for j, path in zip(won, out["win"].select(torch.as_tensor(won * trees + k[won])).moves()):
                solution[j] = path
    return {"visits": visits, "wins": wins, "losses": losses, "best_action": best, "solution": solution,
            "status": out["status"].reshape(M, trees), "tree": out}


ILLEGAL_ACTION = 255   # an action value no state accepts (any value above 3 is illegal)


def actions_from_points(start, points):
    """A path given as points, the dataset's solution format (a list of ``(x, y)`` or of
    ``{'x': .., 'y': ..}`` dicts, the first one the puzzle's start), as the actions that walk it:
    0 right (x + 1), 1 up (y - 1), 2 left (x - 1), 3 down (y + 1), the step's order in
    SPaRC_Gym.py:1131-1188.  A step that is not a unit move (a diagonal, a jump, a repeated point)
    becomes action 255, which no state accepts.  Pure numpy.

    Returns ``(actions, starts_ok)``: ``actions`` uint8 [len(points) - 1] (empty for fewer than two
    points) and whether the first point is ``start`` (True for an empty list: nothing contradicts
    it)."""
    pts = np.asarray([(p["x"], p["y"]) if isinstance(p, dict) else (p[0], p[1]) for p in points], np.int64)
    pts = pts.reshape(-1, 2)
    starts_ok = len(pts) == 0 or (int(pts[0, 0]), int(pts[0, 1])) == (int(start[0]), int(start[1]))
    if len(pts) < 2:
        return np.zeros(0, np.uint8), starts_ok
    dx, dy = np.diff(pts[:, 0]), np.diff(pts[:, 1])
    acts = np.full(len(pts) - 1, ILLEGAL_ACTION, np.uint8)
    for a, (mx, my) in enumerate(((1, 0), (0, -1), (-1, 0), (0, 1))):
        acts[(dx == mx) & (dy == my)] = a
    return acts, starts_ok


def score_paths(vec, puzzle_indices, paths, as_points=False):
    """The puzzle's verdict on proposed paths, any number of them on any puzzles: path ``k`` is
    walked from the reset state of puzzle ``puzzle_indices[k]`` in ONE ``vec.replay`` launch from
    ``vec.roots`` with both stop flags (it ends at its first illegal action, which is not taken, or
    with the step that terminates or truncates), and the end states that terminated are judged by
    ``vec.audit_records``.  ``paths``: per path its actions, or with ``as_points`` its points
    (``actions_from_points``; a path whose first point is not the puzzle's start is replaced by
    the single action 255, so it is refused at index 0 without a step).  Touches no env and does
    not depend on ``vec.num_envs``.

    Returns a dict of numpy arrays [K]: ``end`` (``_lib.REPLAY_END_*``), ``steps``, ``first_bad``
    (the index of the refused action, -1 if none), ``reached`` (ended terminated, on the target,
    with every action consumed), ``listed`` (the last step's reward code was +100: the path is in
    the puzzle's solution list), ``bits`` int64 (the rule bits of the end state, 0 where it was not
    audited) and ``satisfied`` (``bits & RULE_ALL``)."""
    from . import _lib
    q = np.asarray(puzzle_indices, np.int64)
    K = len(paths)
    if q.ndim != 1 or len(q) != K or K < 1:
        raise ValueError("puzzle_indices and paths must hold the same number (at least one) of entries")
    seqs = []
    for k, path in enumerate(paths):
        if as_points:
            acts, ok = actions_from_points(vec.puzzles[int(q[k])]["start_location"], path)
            if not ok:
                acts = np.array([ILLEGAL_ACTION], np.uint8)
        else:
            acts = np.asarray(path, np.int64).reshape(-1)
            if ((acts < 0) | (acts > 255)).any():
                raise ValueError(f"path {k}: actions must be in 0..255")
            acts = acts.astype(np.uint8)
        seqs.append(acts)
    lengths = np.array([len(s) for s in seqs], np.int64)
    L = max(int(lengths.max()), 1)
    actions = np.full((L, K), ILLEGAL_ACTION, np.uint8)
    for k, s in enumerate(seqs):
        actions[:len(s), k] = s
    out = vec.replay(vec.roots(q), actions, lengths=lengths, stop_done=True, stop_illegal=True)
    end = out["end"].cpu().numpy().astype(np.int64)
    steps = out["steps"].cpu().numpy().astype(np.int64)
    bad = out["bad"].cpu().numpy().astype(np.int64)
    code = out["reward_code"].cpu().numpy().astype(np.int64)
    term = end == _lib.REPLAY_END_TERMINATED
    bits = np.zeros(K, np.int64)
    if term.any():
        rows = np.nonzero(term)[0]
        got = vec.audit_records(out["final"].select(rows))["bits"].to(torch.int64) & 0xFFFF
        bits[rows] = got.cpu().numpy()
    return {"end": end, "steps": steps, "first_bad": np.where(bad == 0xFFFF, -1, bad),
            "reached": term & (steps == lengths), "listed": code == 100, "bits": bits,
            "satisfied": (bits & RULE_ALL) != 0}


def solution_dataset(vec, puzzle_indices=None, dtype=torch.uint8):
    """The behaviour-cloning set of the listed solutions: one row per move of every path of
    ``vec.puzzles[q]['solution_paths']`` for ``q`` in ``puzzle_indices`` (default: every puzzle),
    the observation of the state BEFORE the move with the move as its label.  A path is taken when
    it starts at the puzzle's start and consists of unit moves (``actions_from_points``); the
    taken paths are walked in ONE ``vec.replay`` launch from ``vec.roots`` with ``states=True`` (both
    stop flags: a path that replay does not walk to its last point is left out), the record before
    each action (the root, then the states) is gathered, and ONE ``vec.observe`` turns them into
    planes of ``dtype``.  Touches no env and does not depend on ``vec.num_envs``.

    Returns a dict: the observation of ``vec.observe`` over the R rows (``visited``,
    ``agent_location`` [R, x_dim, y_dim], ``puzzle_index``, ``agent_xy``, ``legal_actions``),
    ``action`` [R] uint8 the move taken from that state, ``path`` and ``t`` [R] int64 (which kept
    path, which of its moves; rows are ordered by path, then t), all GPU tensors, and on the host
    ``paths``: per kept path ``(puzzle index, index in its solution list)``, and ``skipped``: the
    counts of listed paths left out, by reason (``wrong_start``, ``non_unit_move``, ``refused``).
    With no move to learn from (no kept path longer than one point) the tensors are None."""
    from .snapshot import Snapshot
    P = len(vec.puzzles)
    qs = np.arange(P) if puzzle_indices is None else np.asarray(puzzle_indices, np.int64).reshape(-1)
    if len(qs) and (int(qs.min()) < 0 or int(qs.max()) >= P):
        raise ValueError(f"puzzle_indices must be in 0..{P - 1}")
    skipped = {"wrong_start": 0, "non_unit_move": 0, "refused": 0}
    cand = []                                            # (puzzle, index in its list, actions)
    for q in qs.tolist():
        p = vec.puzzles[q]
        for s, pts in enumerate(p["solution_paths"]):
            acts, ok = actions_from_points(p["start_location"], pts)
            if not ok:
                skipped["wrong_start"] += 1
            elif (acts == ILLEGAL_ACTION).any():
                skipped["non_unit_move"] += 1
            else:
                cand.append((q, s, acts))
    empty = {k: None for k in ("visited", "agent_location", "puzzle_index", "agent_xy", "legal_actions", "action",
                               "path", "t")}
    walk = [c for c in cand if len(c[2])]                # a one-point path has no move: kept, no row
    kept = [c for c in cand if not len(c[2])]
    if walk:
        K = len(walk)
        lengths = np.array([len(c[2]) for c in walk], np.int64)
        L = int(lengths.max())
        actions = np.full((L, K), ILLEGAL_ACTION, np.uint8)
        for k, c in enumerate(walk):
            actions[:len(c[2]), k] = c[2]
        roots = vec.roots(np.array([c[0] for c in walk], np.int64))
        out = vec.replay(roots, actions, lengths=lengths, stop_done=True, stop_illegal=True, final=False,
                         states=True)
        walked = out["steps"].cpu().numpy().astype(np.int64) == lengths
        skipped["refused"] = int((~walked).sum())
        good = np.nonzero(walked)[0]
        kept += [walk[k] for k in good]
    else:
        good = np.zeros(0, np.int64)
    paths = [(c[0], c[1]) for c in kept]
    if not len(good):
        return {**empty, "paths": paths, "skipped": skipped}
    first = len(kept) - len(good)                        # the kept paths without a move come first
    n = lengths[good]
    path = np.repeat(np.arange(len(good)), n)
    t = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    col = good[path]
    # the record before action t of sequence col: root col (t = 0), else states row (t - 1) * K + col
    row = np.where(t == 0, col, K + (t - 1) * K + col)
    snap = Snapshot.cat([roots, out["states"]]).select(row)
    obs = vec.observe(snap, dtype=dtype)
    dev = obs["visited"].device
    obs["action"] = torch.from_numpy(actions[t, col].copy()).to(dev)
    obs["path"] = torch.from_numpy(path + first).to(dev)
    obs["t"] = torch.from_numpy(t).to(dev)
    obs["paths"] = paths
    obs["skipped"] = skipped
    return obs


def solve_dfs(vec, puzzle_indices, min_roots=4096, budget=4096, max_nodes=None, undecided=65536):
    """Every self-avoiding path from the start of each of ``puzzle_indices`` (one root per entry:
    that puzzle's reset state, all roots at once) counted with the puzzle's own verdict, as
    ``solve_by_rules`` finds them, but depth-first on the GPU (``vec.dfs``, k_dfs): the memory does
    not grow with the tree, so lattices whose levels no frontier can hold are searched too.

    *Split*: forward-only levels of ``expand_frontier`` (the pops dropped, as in ``solve_by_rules``)
    until the frontier holds at least ``min_roots`` nodes or is empty; target nodes met on the way
    are audited with ``vec.audit_records``, dead ends and truncations counted.  *Search*:
    ``vec.dfs`` on the whole frontier with ``budget`` nodes per sub-root and launch, until every
    sub-root is done or, with ``max_nodes`` (anytime mode), the nodes entered reach it.  After each
    launch the undecided leaves (exact fits past the GPU's node cap; at most ``undecided`` stored
    per launch, walks that did not fit resume at their leaf) are judged by ``vec.audit_records``,
    which finishes them on the host, and their verdicts added.  ``undecided=0``: such leaves stay
    in the ``undecided`` counter.

    ``solve_dfs_pruned`` is the same search over the moves that can still reach the target.

    Needs a traceback env with ``max_steps`` at least the lattice's points (ValueError), at least
    ``len(puzzle_indices)`` envs, and overwrites the env state (the roots come from ``vec.reset``).

    Returns a dict, index r: ``puzzle_indices[r]``: ``nodes``, ``targets``, ``satisfied``,
    ``listed``, ``both``, ``dead_ends``, ``truncated``, ``undecided`` int64 [R] (the counters of
    ``vec.dfs`` over the whole tree of root r), ``complete`` [R] bool, ``solution``: the
    lexicographically least satisfying action list from the puzzle's start found so far, or None
    (final when ``complete``), ``launches``: the ``vec.dfs`` calls made, and ``sub_roots``: the
    frontier the search started from."""
    return _solve_dfs(vec, puzzle_indices, min_roots, budget, max_nodes, undecided, 0)


def solve_dfs_pruned(vec, puzzle_indices, min_roots=4096, budget=4096, max_nodes=None, undecided=65536, prune=True):
    """``solve_dfs`` over the moves through which the target can still be reached: the split uses
    ``expand_frontier(..., prune=True)`` and the search ``vec.dfs(..., prune=True)``.  Arguments and
    result as ``solve_dfs``; ``prune``: True or "reach" (False: ``solve_dfs`` itself).  The counters
    are those of the pruned walk from each puzzle's start: ``solution`` and ``targets``,
    ``satisfied``, ``listed``, ``both``, ``undecided`` equal ``solve_dfs``'s, ``nodes`` is smaller,
    and ``dead_ends`` is 1 for a start that is walled off from its target and 0 otherwise (a node the
    split cuts is not a dead end, it is never entered).  ``max_steps`` is at least the lattice's
    points here, so the deadline mode of ``vec.dfs`` would cut nothing more (ValueError)."""
    from . import _lib
    mode = _lib.dfs_prune_mode(prune)
    if mode not in (0, _lib.DFS_PRUNE_REACH):
        raise ValueError('solve_dfs_pruned prunes by reach only: prune must be False, True or "reach"')
    return _solve_dfs(vec, puzzle_indices, min_roots, budget, max_nodes, undecided, mode)


def _solve_dfs(vec, puzzle_indices, min_roots, budget, max_nodes, undecided, mode):
    """solve_dfs (mode 0) and solve_dfs_pruned (mode 1, _lib.DFS_PRUNE_REACH)."""
    from . import _lib
    q = np.asarray(puzzle_indices, np.int64)
    R = len(q)
    if q.ndim != 1 or R < 1 or R > vec.num_envs:
        raise ValueError(f"puzzle_indices must hold 1..{vec.num_envs} puzzle indices")
    if not vec.traceback:
        raise ValueError("solve_dfs needs a traceback env: the record's direction stack is the search stack")
    points = max(int(vec.puzzles[int(k)]["x_size"]) * int(vec.puzzles[int(k)]["y_size"]) for k in q)
    if vec.max_steps < points:
        raise ValueError(f"max_steps = {vec.max_steps} is below the lattice's {points} points: paths would be "
                         "truncated")
    full = np.full(vec.num_envs, q[0], np.int64)
    full[:R] = q
    vec.reset(options={"puzzle_index": full})
    frontier = vec.snapshot(envs=np.arange(R))
    dev = frontier.records.device
    root = torch.arange(R, device=dev)
    C = _lib.DFS_COUNTERS
    total = torch.zeros((R, C), dtype=torch.int64, device=dev)
    best = [None] * R

    def add(col, roots, weight=None):
        if len(roots):
            total[:, col] += torch.bincount(roots, weights=weight, minlength=R).to(torch.int64)

    def offer(snap, roots):                               # satisfying leaves: candidates for the solution
        for r, m in zip(roots.cpu().numpy(), snap.moves()):
            if best[int(r)] is None or m < best[int(r)]:
                best[int(r)] = m

    def judge(snap, roots, listed):                       # final verdicts of target records
        bits = vec.audit_records(snap)["bits"].to(torch.int64) & 0xFFFF
        sat = (bits & RULE_ALL) != 0
        add(_lib.DFS_SATISFIED, roots[sat])
        add(_lib.DFS_BOTH, roots[sat & listed])
        rows = sat.nonzero().squeeze(1)
        if len(rows):
            offer(snap.select(rows), roots[rows])

    # ---- split: forward-only breadth-first levels
    while 0 < len(frontier) < min_roots:
        out = expand_frontier(vec, frontier, prune=mode != 0)   # the frontier holds live nodes only
        children, parent = out["children"], out["parent"]
        code, flags = out["reward_code"], out["flags"]
        if len(children):                                 # drop the pops: one point shorter than the parent
            fwd = children.fields()["path_len"] > frontier.fields()["path_len"][parent]
            keep = fwd.nonzero().squeeze(1)
            children, parent, code, flags = children.select(keep), parent[keep], code[keep], flags[keep]
        kids = torch.bincount(parent, minlength=len(frontier))
        add(_lib.DFS_DEAD_ENDS, root[kids == 0])          # live without a forward move (pruned: a start only)
        if len(children) == 0:
            frontier = children
            root = root[:0]
            break
        croot = root[parent]
        add(_lib.DFS_NODES, croot)
        term = (flags & TERMINATED) != 0
        rows = term.nonzero().squeeze(1)
        if len(rows):
            listed = code[rows] == 100
            add(_lib.DFS_TARGETS, croot[rows])
            add(_lib.DFS_LISTED, croot[rows][listed])
            judge(children.select(rows), croot[rows], listed)
        add(_lib.DFS_TRUNCATED, croot[((flags & DONE_BITS) != 0) & ~term])
        live = ((flags & DONE_BITS) == 0).nonzero().squeeze(1)
        frontier = children.select(live)
        root = croot[live]
    # ---- search: depth-first below every node of the frontier
    M = len(frontier)
    complete = np.ones(R, np.bool_)
    launches = 0
    if M:
        cur, state, counts, first = frontier, None, None, None
        resolved = torch.zeros(M, dtype=torch.int64, device=dev)
        split_nodes = int(total[:, _lib.DFS_NODES].sum())
        while True:
            out = vec.dfs(cur, budget, state=state, counts=counts, first=first, undecided=undecided,
                          prune=mode != 0)
            launches += 1
            cur, state, counts, first = out["cursor"], out["state"], out["counts"], out["first"]
            if undecided and len(out["undecided"]):
                und, sub = out["undecided"], out["undecided_root"]
                aux = und.records[:, 4:8].to(torch.int64)
                listed = ((aux[:, 2] & 3) == 1)           # outcome +1: the step's code was +100
                judge(und, root[sub], listed)
                resolved += torch.bincount(sub, minlength=M)
            if bool(out["done"].all()):
                break
            if max_nodes is not None and split_nodes + int(counts[:, _lib.DFS_NODES].sum()) >= max_nodes:
                break
        total.index_add_(0, root, counts)
        add(_lib.DFS_UNDECIDED, root, -resolved.to(torch.float64))
        found = out["found"].nonzero().squeeze(1)
        if len(found):
            offer(first.select(found), root[found])
        open_roots = root[~out["done"]].cpu().numpy()
        complete[open_roots] = False
    res = {name: total[:, k].cpu().numpy() for k, name in enumerate(_lib.DFS_COUNTER_NAMES)}
    res.update(complete=complete, solution=best, launches=launches, sub_roots=M)
    return res


def solve_by_rules(vec, puzzle_indices, max_frontier=1 << 22, prune=False):
    """Every self-avoiding path from the start to the target of each of ``puzzle_indices`` (one
    root per entry: that puzzle's reset state, all roots at once), with the puzzle's own verdict on
    it: the rule audit of the state the path ends in (``vec.audit_records``), beside the verdict of
    the stored solution list (the last step's reward code).

    The tree of forward moves is walked breadth-first with ``expand_frontier``.  On a traceback
    env the legal moves include the pop back to the previous point; those children (one point
    shorter than their parent, ``Snapshot.fields()['path_len']``) are dropped, so the tree is the
    same with and without traceback.  A node whose step terminated has reached the target
    (SPaRC_Gym.py:1192): these are the only states for which ``all_rules_satisfied`` can hold
    (931-950), and the only ones audited.  A path has fewer moves than the lattice has points, so
    ``vec.max_steps`` must be at least that (ValueError otherwise: a truncation would cut paths
    short silently).  RuntimeError if a level holds more than ``max_frontier`` nodes.

    The roots come from ``vec.reset`` and ``vec.snapshot``, so ``vec`` needs at least
    ``len(puzzle_indices)`` envs and its state is overwritten.

    Returns a dict of per-root lists (index r: ``puzzle_indices[r]``), paths in ascending (depth,
    frontier row) order: ``paths`` the action sequences that reach the target, ``bits`` [K_r] int64
    their rule bits, ``satisfied`` [K_r] bool (``bits & RULE_ALL``), ``listed`` [K_r] bool (the last
    step's reward code was +100: the path is in the puzzle's solution list); and ``nodes`` int64
    [R, D + 1], the forward-move nodes at each depth (column 0: the roots).  Nothing asserts that
    ``satisfied`` and ``listed`` agree: that is a fact about a dataset.

    ``prune=True`` walks with ``expand_frontier(..., prune=True)``: a child from which the target
    cannot be reached any more has no target node below it, so ``paths``, ``bits``, ``satisfied``
    and ``listed`` are the same, in the same order, and only ``nodes`` gets smaller."""
    q = np.asarray(puzzle_indices, np.int64)
    R = len(q)
    if q.ndim != 1 or R < 1 or R > vec.num_envs:
        raise ValueError(f"puzzle_indices must hold 1..{vec.num_envs} puzzle indices")
    points = max(int(vec.puzzles[int(k)]["x_size"]) * int(vec.puzzles[int(k)]["y_size"]) for k in q)
    if vec.max_steps < points:
        raise ValueError(f"max_steps = {vec.max_steps} is below the lattice's {points} points: paths would be "
                         "truncated")
    full = np.full(vec.num_envs, q[0], np.int64)
    full[:R] = q
    vec.reset(options={"puzzle_index": full})
    frontier = vec.snapshot(envs=np.arange(R))
    dev = frontier.records.device
    root = torch.arange(R, device=dev)
    nodes = [np.ones(R, np.int64)]
    levels = []                                          # per level: parent, action, live rows
    hits = []                                            # per level: (rows, roots, bits, listed) of its target nodes
    while len(frontier):
        out = expand_frontier(vec, frontier, prune=prune)   # the frontier holds live nodes only
        children, parent, action = out["children"], out["parent"], out["action"]
        code, flags = out["reward_code"], out["flags"]
        if vec.traceback and len(children):              # drop the pops: one point shorter than the parent
            fwd = children.fields()["path_len"] > frontier.fields()["path_len"][parent]
            keep = fwd.nonzero().squeeze(1)
            children, parent, action = children.select(keep), parent[keep], action[keep]
            code, flags = code[keep], flags[keep]
        K = len(children)
        if K == 0:
            break
        if K > max_frontier:
            raise RuntimeError(f"depth {len(nodes)} holds {K} nodes, more than max_frontier = {max_frontier}")
        croot = root[parent]
        nodes.append(torch.bincount(croot, minlength=R).cpu().numpy().astype(np.int64))
        rows = ((flags & TERMINATED) != 0).nonzero().squeeze(1)
        if len(rows):
            bits = vec.audit_records(children.select(rows))["bits"].to(torch.int64) & 0xFFFF
            hits.append((rows.cpu().numpy(), croot[rows].cpu().numpy(), bits.cpu().numpy(),
                         (code[rows] == 100).cpu().numpy()))
        else:
            hits.append(None)
        live = ((flags & DONE_BITS) == 0).nonzero().squeeze(1)
        levels.append((parent.cpu().numpy(), action.cpu().numpy(), live.cpu().numpy()))
        frontier = children.select(live)
        root = croot[live]
    paths = [[] for _ in range(R)]
    bits_r, listed_r = [[] for _ in range(R)], [[] for _ in range(R)]
    for d, h in enumerate(hits, start=1):
        if h is None:
            continue
        rows, roots, bits, listed = h
        acts = np.empty((len(rows), d), np.int64)        # walk all of the level's target nodes back at once
        row = rows.copy()
        for lv in range(d, 0, -1):
            par, act, _ = levels[lv - 1]
            acts[:, lv - 1] = act[row]
            prow = par[row]                              # rows of the frontier expanded at level lv
            row = prow if lv == 1 else levels[lv - 2][2][prow]
        for k in range(len(rows)):
            r = int(roots[k])
            paths[r].append([int(a) for a in acts[k]])
            bits_r[r].append(int(bits[k]))
            listed_r[r].append(bool(listed[k]))
    bits_r = [np.asarray(b, np.int64) for b in bits_r]
    return {"paths": paths, "bits": bits_r, "satisfied": [(b & RULE_ALL) != 0 for b in bits_r],
            "listed": [np.asarray(v, np.bool_) for v in listed_r], "nodes": np.stack(nodes, 1)}
