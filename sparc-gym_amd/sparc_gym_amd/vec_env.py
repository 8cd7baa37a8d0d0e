"""SPaRCVecEnv: thousands of SPaRC envs stepped together on one MI355X.

The batched form of the reference's ``reset()/step()`` (SPaRC_Gym.py:1057-1238).  State lives in
HBM as a structure of arrays owned by the C context; every call is one HIP launch on the
caller's torch stream, and results stay on the GPU as torch tensors (no host round trip).

    vec = SPaRCVecEnv(65536, puzzles=records, traceback=True)
    obs, info = vec.reset(seed=0)
    obs, reward, terminated, truncated, info = vec.step(actions)   # actions: [N] on the GPU
    out = vec.rollout(T, actions=None, seed=1)                      # T steps in one launch

Autoreset follows gymnasium's next-step convention by default: the step after an env
terminates/truncates resets it onto the next puzzle ((index + 1) % P, the reference's plain
``reset()`` at SPaRC_Gym.py:1087) and ignores that step's action.  ``autoreset='none'``
reproduces the reference exactly (stepping past the end keeps the finished state).

Observations (``observation='new'``): ``visited`` and ``agent_location`` as int32 planes
[N, x_dim, y_dim] (padded lattice) written by the obs-pack kernel, plus ``puzzle_index``; the
static planes (gaps, target, symbols, color, additional_info) of every puzzle are in
``static_planes`` and ``static_keys`` (``static_planes[puzzle_index]`` gives an env's).
``observation='compact'`` returns only ``puzzle_index`` and the agent location.

Rule audit (``rules=True``, or ``rule_audit()`` on demand): the reference's
``info['rule_status']`` (SPaRC_Gym.py:941-950) evaluated by the k_rules kernel for every env,
as ``info['rule_bits']`` [N] int16 with bit k = ``RULE_NAMES[k]`` passed.  An exact-fit search
that passes the GPU's node cap (``fit_cap``, default 2^26) is finished on the host without a
cap, as the reference's unbounded search (sparc_rules_finish): the bits are always final.

Snapshot / restore / fork: ``snapshot()`` returns the state of any envs as opaque records
(``sparc_gym_amd.Snapshot``), ``restore(snap, src, mask)`` writes record ``src[i]`` into env ``i``
of any env on the same puzzle table, ``fork(src)`` makes env ``i`` a copy of env ``src[i]``: one
position fanned out to every env for playouts, beam search or MCTS, or a run saved and resumed.
``expand(snap)`` returns all four successors of any number of records in one launch without
touching an env (the one-ply step of a tree search; ``sparc_gym_amd.search`` builds on it).
``playout(snap, K, L)`` plays K random legal-move continuations of every record to the end of
its episode or L steps, again in one launch without an env, with per-root statistics
(``search.monte_carlo``).  ``replay(snap, actions, lengths)`` plays action sequences that the caller
supplies, from records or (``puzzle_indices``) from puzzles' reset states, again in one launch without
an env; ``roots(puzzle_indices)`` gives reset states as records (``search.score_paths``).
``observe(snap, dtype, out, channels)`` returns the observation ``step()`` returns for records instead
of envs: the ``visited`` and ``agent_location`` planes in the network's dtype, optionally straight
into two channels of the network's input tensor, with ``puzzle_index``, ``agent_xy`` and
``legal_actions``, again in one launch without an env (``search.solution_dataset``).
``reach(snap, plane)`` tells for records whether the free lattice points still connect the agent to the
target, the distance to it overall and through each action, and optionally the distance plane, again in
one launch without an env (``search.expand_frontier(..., prune=True)``).
``mcts(snap, sims, horizon)`` grows a UCT search tree per record, kept on the GPU between calls and
resumable, again in one launch without an env (``search.uct``).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .core import SparcCore
from .env import load_puzzle_source
from .puzzles import pack_rules, pack_table, process_puzzles

RULE_NAMES = ("reached_target", "path_not_crossing", "no_gap_violations", "all_dots_collected",
              "square_color_separation", "star_pairing_exact", "triangles_edge_count", "poly_ylop_area",
              "all_rules_satisfied")   # _run_rule_validators order, SPaRC_Gym.py:908-936

# reward code -> float64 value; code/100 in float64 is exactly the reference's 0.01/-0.01 double
REWARD_SCALE = 100.0


def xcd_local_puzzle_index(num_envs, num_puzzles, env_offset=0):
    """First puzzles for a batched reset (``reset(options={'puzzle_index': ...})``) that keep each
    XCD's L2 on one eighth of a large pool.  The split rollout kernel runs 256 envs per workgroup
    and the MI355X deals workgroups round-robin over its 8 XCDs (workgroups b, b + 8, ... share
    one XCD and its 4 MB L2), so env slot s belongs to XCD group g = (s // 256) % 8; it gets a
    puzzle of block g of the pool, [g * P/8, (g+1) * P/8), by a multiplicative hash of its index
    within the group (plus env_offset, so shards differ).  Every puzzle starts equally many envs
    (num_envs a multiple of 2,048 and P of 8); next-step autoresets walk on from the start
    puzzle (reset(), SPaRC_Gym.py:1087).  With env i on puzzle i * 2654435761 mod P every XCD
    touches the whole pool instead (MI355X, c3 at 16,384 puzzles: 0.353 against 0.404 ms per
    2,000-step launch; the library then also keeps the shorter 8-B trie records,
    sparc_reset_host).  P < 8 or P % 8 != 0: the plain hash."""
    P = int(num_puzzles)
    slot = np.arange(int(num_envs), dtype=np.uint64)
    if P < 8 or P % 8:
        return ((slot + np.uint64(env_offset)) * np.uint64(2654435761) % np.uint64(P)).astype(np.int64)
    span = np.uint64(P // 8)
    grp = (slot // np.uint64(256)) % np.uint64(8)
    k = (slot // np.uint64(2048)) * np.uint64(256) + slot % np.uint64(256) + np.uint64(env_offset)
    return (grp * span + k * np.uint64(2654435761) % span).astype(np.int64)


class _RecordReplay:
    """``replay`` and ``roots`` of ``SPaRCVecEnv``: the calls that play given actions from records
    or puzzle roots without an env.  A base class of its own: tests/test_stream_binding.py pins the
    methods defined on ``SPaRCVecEnv`` itself to the list its stream tests walk, and
    tests/test_replay_guards.py and tests/test_gpu_replay.py check the same contract (the caller's
    stream is bound before the first call into the core) for these two."""

    def replay(self, snap=None, actions=None, lengths=None, puzzle_indices=None, stop_done=False,
               stop_illegal=False, per_step=False, final=True, states=False):
        """Play given action sequences, one per start state, in one launch and without changing or
        reading any env (k_replay): what the reference's user does with a model's proposed moves
        (step the env with them and read the result, SPaRC_Gym.py:1111-1238), for any number of
        proposals at once.  Sequence ``j`` starts from record ``j`` of ``snap`` or from the reset
        state of puzzle ``puzzle_indices[j]`` (exactly one of the two is given; M starts in all).
        ``actions``: [L, M] uint8 (numpy or tensor), step-major as ``playout``'s trace; ``lengths``
        [M]: the actions of sequence ``j`` (default: L each); every value is an action, 255 and
        everything else above 3 an illegal one.  ``actions=None`` is L = 0: no step, only the start
        records (``roots``).

        Without a stop flag sequence ``j`` is byte for byte ``restore`` of its start, ``lengths[j]``
        ``step`` calls and ``snapshot`` under this env's ``max_steps`` and ``autoreset``: an illegal
        action gives the no-move state with step + 1, and a step after the end steps past it
        (``autoreset='none'``) or loads the next puzzle (flag 64).  ``stop_done``: the sequence ends
        with the step that terminates or truncates (a start that is already done takes no step).
        ``stop_illegal``: an action that is not legal in the current state ends the sequence before
        it is taken.

        Returns a dict of GPU tensors [M]: ``reward_code`` int8 and ``flags`` uint8 of the last step
        taken (0 without one), ``steps`` int32, ``end`` uint8 (``_lib.REPLAY_END_*``: 0 bad start,
        1 terminated, 2 truncated, 3 every action taken, 4 stopped at an illegal action, 5 the start
        was already done), ``return`` int32 the sum of the reward codes, ``bad`` int32 the index of
        the action ``stop_illegal`` refused (65535: none); with ``per_step`` ``step_code`` int8 and
        ``step_flags`` uint8 [L, M], 0 at and after the end; with ``final`` a ``Snapshot`` of the M
        end states; with ``states`` a ``Snapshot`` of ``L * M`` records, row ``t * M + j`` the state
        after step ``t`` of sequence ``j``, zeroed at and after the end (``audit_records`` of it gives
        the reference's per-step ``info['rule_status']``).  A start that fails the kernel's checks
        gives end 0 and zeroed outputs, and the next ``core.sync()`` raises.  ValueError: both or
        neither of ``snap`` and ``puzzle_indices``, a shape or dtype mismatch, host ``lengths``
        above L (a tensor's are clamped by the kernel), a snapshot header that does not match this
        env (naming the field)."""
        from .snapshot import Snapshot, info_mismatch
        self._stream()
        if (snap is None) == (puzzle_indices is None):
            raise ValueError("give exactly one of snap and puzzle_indices")
        if snap is not None:
            M = len(snap)
        elif isinstance(puzzle_indices, torch.Tensor):
            M = int(puzzle_indices.shape[0]) if puzzle_indices.ndim == 1 else 0
        else:
            M = int(np.asarray(puzzle_indices).shape[0]) if np.asarray(puzzle_indices).ndim == 1 else 0
        if not 1 <= M < 2**31:
            raise ValueError("1 .. 2^31 - 1 start states (records or a one-dimensional puzzle_indices) are needed")
        if actions is None:
            L = 0
            if lengths is not None or per_step or states:
                raise ValueError("without actions (L = 0) there are no lengths, per-step outputs or states")
        else:
            if not isinstance(actions, (torch.Tensor, np.ndarray)):
                raise ValueError("actions must be a uint8 numpy array or tensor [L, M]")
            if actions.dtype != (torch.uint8 if isinstance(actions, torch.Tensor) else np.uint8):
                raise ValueError(f"actions must be uint8, not {actions.dtype}")
            if actions.ndim != 2 or actions.shape[1] != M:
                raise ValueError(f"actions must have shape [L, {M}], not {list(actions.shape)}")
            L = int(actions.shape[0])
            if not 1 <= L <= 65535:
                raise ValueError("actions must hold 1..65535 steps (L); pass actions=None for L = 0")
        if lengths is not None and not isinstance(lengths, torch.Tensor):
            lengths = np.asarray(lengths)
            if lengths.shape != (M,) or lengths.dtype.kind not in "iu":
                raise ValueError(f"lengths must be integers of shape ({M},)")
            if int(lengths.min()) < 0 or int(lengths.max()) > L:
                raise ValueError(f"lengths must be in 0..{L} (the rows of actions)")
            lengths = torch.from_numpy(lengths.astype(np.int32))
        elif lengths is not None and (lengths.shape != (M,) or lengths.dtype.is_floating_point or
                                      lengths.dtype == torch.bool):
            raise ValueError(f"lengths must be integers of shape ({M},)")
        pz = None if puzzle_indices is None else self._index_arg(puzzle_indices, "puzzle_indices", self.num_puzzles)
        info = self.core.snapshot_info()
        if snap is not None:
            bad = info_mismatch(snap.info, info)
            if bad is not None:
                raise ValueError(f"snapshot does not match this env: {bad} differs")
            info = snap.info
            rec = snap.records
            if not isinstance(rec, torch.Tensor):
                rec = torch.from_numpy(np.ascontiguousarray(rec, np.uint8))
            rec = rec.to(self.device).contiguous()
        dev = self.device
        act = None
        if L:
            act = actions
            if not isinstance(act, torch.Tensor):
                act = np.ascontiguousarray(act)
                act = torch.from_numpy(act if act.flags.writeable else act.copy())   # (torch wants a writable one)
            act = act.to(dev).contiguous()
        ln = None if lengths is None else lengths.to(device=dev, dtype=torch.int32).contiguous()
        ret = torch.empty(M, dtype=torch.int32, device=dev)
        h = torch.empty((2, M), dtype=torch.int16, device=dev)        # steps | bad
        b = torch.empty((3, M), dtype=torch.uint8, device=dev)        # code | flags | end
        out = {"reward_code": b[0].view(torch.int8), "flags": b[1], "end": b[2], "return": ret}
        if per_step:
            sb = torch.empty((2, L, M), dtype=torch.uint8, device=dev)
            out["step_code"], out["step_flags"] = sb[0].view(torch.int8), sb[1]
        rb = info.record_bytes
        fin = torch.empty((M, rb), dtype=torch.uint8, device=dev) if final else None
        st = torch.empty((L * M, rb), dtype=torch.uint8, device=dev) if states else None
        flags = (_lib.REPLAY_STOP_DONE if stop_done else 0) | (_lib.REPLAY_STOP_ILLEGAL if stop_illegal else 0)
        self.core.replay_device(info, rec.data_ptr() if snap is not None else None,
                                pz.data_ptr() if pz is not None else None, M, L,
                                act.data_ptr() if L else None, ln.data_ptr() if ln is not None else None, flags,
                                d_code=b[0].data_ptr(), d_flags=b[1].data_ptr(), d_steps=h[0].data_ptr(),
                                d_end=b[2].data_ptr(), d_return=ret.data_ptr(), d_bad=h[1].data_ptr(),
                                d_step_code=sb[0].data_ptr() if per_step else None,
                                d_step_flags=sb[1].data_ptr() if per_step else None,
                                d_final=fin.data_ptr() if final else None,
                                d_states=st.data_ptr() if states else None)
        out["steps"] = h[0].to(torch.int32) & 0xFFFF                  # the kernel writes uint16
        out["bad"] = h[1].to(torch.int32) & 0xFFFF
        if final:
            out["final"] = Snapshot(fin, info)
        if states:
            out["states"] = Snapshot(st, info)
        return out

    def roots(self, puzzle_indices):
        """The reset state of every puzzle of ``puzzle_indices`` (any number, repeats allowed) as a
        ``Snapshot``: the records ``reset`` on those puzzles plus ``snapshot`` give (reset(),
        SPaRC_Gym.py:1057-1108), made by ``replay`` with no action, so no env is needed, read or
        written and the env need never have been reset."""
        return self.replay(puzzle_indices=puzzle_indices)["final"]


OBS_DTYPES = {torch.int32: _lib.OBS_I32, torch.uint8: _lib.OBS_U8, torch.float16: _lib.OBS_F16,
              torch.bfloat16: _lib.OBS_BF16, torch.float32: _lib.OBS_F32}


class _RecordObserve:
    """``observe`` of ``SPaRCVecEnv``: the observation of records instead of envs.  A base class of
    its own for the reason ``_RecordReplay`` is one; tests/test_observe_guards.py and
    tests/test_gpu_observe.py check the stream contract for it."""

    def observe(self, snap, dtype=torch.int32, out=None, channels=None):
        """The observation ``step()`` returns (_get_obs, SPaRC_Gym.py:956-979), for the records of
        ``snap`` instead of envs, in one launch and without changing or reading any env
        (k_observe_rec): the input of a policy or value network over a search frontier, the
        children of ``expand`` or the ``states`` of ``replay``.

        Returns a dict of GPU tensors: ``visited`` and ``agent_location`` [M, x_dim, y_dim] of
        ``dtype`` (int32, the reference's; uint8, float16, bfloat16 or float32: 1 / 1.0 and 0), bit
        for bit the planes ``restore`` of the records into M envs and ``reset``'s observation give;
        ``puzzle_index`` [M] int32 (``static_planes[puzzle_index]`` are the static planes);
        ``agent_xy`` [M, 2] int32; ``legal_actions`` [M] uint8, bit a set when action a is legal in
        the record's state (``info['legal_actions']`` of ``restore``).  A pending record is observed
        as it stands.

        ``out``: a contiguous [M, C, x_dim, y_dim] tensor of ``dtype`` on this env's device, with
        ``channels=(c_visited, c_agent)``: the two planes are written straight into those channels
        of it (the network's input, assembled without a copy), the returned planes are views of
        them, and no other byte of ``out`` is touched.

        A record that fails the kernel's checks gets all-zero planes, ``puzzle_index`` -1,
        ``agent_xy`` (0, 0) and ``legal_actions`` 0, and the next ``core.sync()`` raises.
        ValueError: an unsupported ``dtype``, ``out`` without ``channels`` or the reverse, a shape,
        dtype, device or layout mismatch of ``out``, equal or out-of-range channels, a snapshot
        header that does not match this env (naming the field)."""
        from .snapshot import info_mismatch
        self._stream()
        if dtype not in OBS_DTYPES:
            raise ValueError(f"dtype must be one of {sorted(str(d) for d in OBS_DTYPES)}, not {dtype}")
        M = len(snap)
        if not 1 <= M < 2**31:
            raise ValueError("snap must hold 1 .. 2^31 - 1 records")
        X, Y = self.x_dim, self.y_dim
        if (out is None) != (channels is None):
            raise ValueError("out and channels are given together or not at all")
        if out is not None:
            if not isinstance(out, torch.Tensor):
                raise ValueError("out must be a tensor")
            if out.dtype != dtype:
                raise ValueError(f"out must have dtype {dtype}, not {out.dtype}")
            if out.device != self.device:
                raise ValueError(f"out must be on device {self.device}, not {out.device}")
            if out.ndim != 4 or out.shape[0] != M or out.shape[1] < 2 or tuple(out.shape[2:]) != (X, Y):
                raise ValueError(f"out must have shape [{M}, C >= 2, {X}, {Y}], not {list(out.shape)}")
            if not out.is_contiguous():
                raise ValueError("out must be contiguous")
            try:
                cv, ca = (int(c) for c in channels)
            except (TypeError, ValueError):
                raise ValueError("channels must be two integers (c_visited, c_agent)") from None
            C = int(out.shape[1])
            if not (0 <= cv < C and 0 <= ca < C) or cv == ca:
                raise ValueError(f"channels must be two different values in 0..{C - 1}")
        info = self.core.snapshot_info()
        bad = info_mismatch(snap.info, info)
        if bad is not None:
            raise ValueError(f"snapshot does not match this env: {bad} differs")
        rec = snap.records
        if not isinstance(rec, torch.Tensor):
            rec = torch.from_numpy(np.ascontiguousarray(rec, np.uint8))
        rec = rec.to(self.device).contiguous()
        dev = self.device
        if out is None:
            planes = torch.empty((2, M, X, Y), dtype=dtype, device=dev)
            vis, agent, stride = planes[0], planes[1], 0
        else:
            vis, agent, stride = out[:, cv], out[:, ca], C * X * Y
        pidx = torch.empty(M, dtype=torch.int32, device=dev)
        loc = torch.empty((M, 2), dtype=torch.int32, device=dev)
        legal = torch.empty(M, dtype=torch.uint8, device=dev)
        self.core.observe_records_device(snap.info, rec.data_ptr(), M, OBS_DTYPES[dtype], X, Y, stride,
                                         d_visited=vis.data_ptr(), d_agent=agent.data_ptr(),
                                         d_puzzle=pidx.data_ptr(), d_loc=loc.data_ptr(), d_legal=legal.data_ptr())
        return {"visited": vis, "agent_location": agent, "puzzle_index": pidx, "agent_xy": loc,
                "legal_actions": legal}


REACH_NONE = _lib.REACH_NONE


class _RecordReach:
    """``reach`` of ``SPaRCVecEnv``: target reachability and distances of records.  A base class of
    its own for the reason ``_RecordReplay`` is one; tests/test_reach_guards.py and
    tests/test_gpu_reach.py check the stream contract for it."""

    def reach(self, snap, plane=False):
        """Can each record of ``snap`` still reach its puzzle's target, and how far away is it: a
        flood of the lattice points the path has left free, from the target, in one launch and
        without changing or reading any env (k_reach_rec).  A path is self-avoiding, so a record
        the path has walled off from the target is lost whatever the rules say, and so is every
        record below it.

        Returns a dict of GPU uint8 tensors, ``REACH_NONE`` (255) standing for "no way":
        ``dist`` [M], 0 on the target, else the moves still needed at least; ``action_dist``
        [M, 4], the same through each action (exactly ``dist`` of that child of ``expand``, plus
        1); ``live`` [M], bit a set when action a keeps the target reachable, a subset of the
        forward legal moves; ``size`` [M], the number of free points connected to the target; with
        ``plane=True`` also ``plane`` [M, x_dim, y_dim], the distance to the target of every such
        point and 255 elsewhere (an input channel, or a shaping potential).  Only the puzzle, the
        agent's point and the visited board of a record enter; a pending record is answered as it
        stands.

        A record that fails the kernel's checks gets ``dist`` and ``action_dist`` 255, ``live`` 0,
        ``size`` 0 and a plane of 255, and the next ``core.sync()`` raises.  ValueError: an empty
        ``snap``, a snapshot header that does not match this env (naming the field)."""
        from .snapshot import info_mismatch
        self._stream()
        M = len(snap)
        if not 1 <= M < 2**31:
            raise ValueError("snap must hold 1 .. 2^31 - 1 records")
        info = self.core.snapshot_info()
        bad = info_mismatch(snap.info, info)
        if bad is not None:
            raise ValueError(f"snapshot does not match this env: {bad} differs")
        rec = snap.records
        if not isinstance(rec, torch.Tensor):
            rec = torch.from_numpy(np.ascontiguousarray(rec, np.uint8))
        rec = rec.to(self.device).contiguous()
        dev, X, Y = self.device, self.x_dim, self.y_dim
        out = {"dist": torch.empty(M, dtype=torch.uint8, device=dev),
               "action_dist": torch.empty((M, 4), dtype=torch.uint8, device=dev),
               "live": torch.empty(M, dtype=torch.uint8, device=dev),
               "size": torch.empty(M, dtype=torch.uint8, device=dev)}
        if plane:
            out["plane"] = torch.empty((M, X, Y), dtype=torch.uint8, device=dev)
        self.core.reach_records_device(snap.info, rec.data_ptr(), M, X, Y, d_dist=out["dist"].data_ptr(),
                                       d_action_dist=out["action_dist"].data_ptr(), d_live=out["live"].data_ptr(),
                                       d_size=out["size"].data_ptr(),
                                       d_plane=out["plane"].data_ptr() if plane else None)
        return out


def uct_tables(c=1.0, entries=4096):
    """The default exploration tables of ``mcts``: ``ep[n] = c * sqrt(ln max(n, 1))`` over the
    node's visits and ``ec[n] = 1 / sqrt(max(n, 1))`` over the child's, so that ``ep * ec`` is UCT's
    ``c * sqrt(ln N / n)``; computed in float64, then rounded to float32.  Indices past the last
    entry read the last one.  Returns two numpy float32 arrays [entries]."""
    entries = int(entries)
    if entries < 2:
        raise ValueError("entries must be at least 2")
    n = np.maximum(np.arange(entries, dtype=np.float64), 1.0)
    return (float(c) * np.sqrt(np.log(n))).astype(np.float32), (1.0 / np.sqrt(n)).astype(np.float32)


class _RecordMcts:
    """``mcts`` of ``SPaRCVecEnv``: the UCT tree search of records.  A base class of its own for the
    reason ``_RecordReplay`` is one; tests/test_mcts_guards.py and tests/test_gpu_mcts.py check the
    stream contract for it."""

    def mcts(self, snap, sims, horizon, c=1.0, explore=None, tree=None, cap=None, seed=0, id0=0, forward_only=None):
        """``sims`` UCT simulations on a search tree of every record of ``snap`` (M roots), in one
        launch and without changing or reading any env (k_mcts): selection by
        ``wins / n + ep[visits] * ec[n]`` over the forward moves (the legal actions without the
        traceback pop, ``dfs``'s children), one new node per simulation, a legal-move rollout of at
        most ``horizon`` steps from it (``playout``'s, drawn with id ``id0 + j * 2**32 + s`` for
        simulation ``s`` of root ``j``; ``forward_only``, by default ``self.traceback``, keeps the
        pop out of it), and the backup of the last step's reward code (+100 a win, -100 a loss).

        ``explore=(ep, ec)``: two float32 tables of the same length T >= 2, finite, indexed by
        ``min(visits, T - 1)`` of the node and ``min(n, T - 1)`` of the child; default
        ``uct_tables(c)``.  ``tree``: the dict a previous call returned, to continue its trees (same
        ``snap``; k calls of S simulations give what one call of k * S gives, byte for byte).
        ``cap``: the nodes per root of a fresh arena (default ``sims + 1``, which is always enough),
        or of a larger arena the given tree is copied into first.

        Returns a dict on the GPU: ``status`` [M] uint8 (``_lib.MCTS_*``: 0 refused, 1 done, 2 the
        arena is full or the root's visits are at their limit, 3 the record was already done, 4 it
        is live without a forward move), ``sims`` [M] int32 the simulations of this call,
        ``nodes`` [M, cap, 16] uint32 and ``count`` [M] int32 the trees (the node layout:
        INTEGRATION.md), ``win`` a ``Snapshot`` of the shortest winning end state per root and
        ``win_steps`` [M] int64 its steps from the root, -1 where none was found (``win`` is zeroed
        there).  A root that fails the kernel's checks (a bad record, a damaged tree) gets status 0,
        and the next ``core.sync()`` raises.  ValueError naming the argument otherwise."""
        from .snapshot import Snapshot, info_mismatch
        self._stream()
        bad = info_mismatch(snap.info, self.core.snapshot_info())
        if bad is not None:
            raise ValueError(f"snapshot does not match this env: {bad} differs")
        M, sims, L = len(snap), int(sims), int(horizon)
        if forward_only is None:
            forward_only = bool(self.traceback)
        dev, rb = self.device, snap.info.record_bytes
        if tree is None:
            cap = sims + 1 if cap is None else int(cap)
        else:
            old = tree["nodes"]
            if not (isinstance(old, torch.Tensor) and old.dtype == torch.uint32 and old.ndim == 3 and
                    old.shape[0] == M and old.shape[2] == _lib.MCTS_NODE_WORDS and old.is_contiguous() and
                    old.device == dev):
                raise ValueError(f"tree['nodes'] must be a contiguous uint32 tensor [{M}, cap, 16] on {dev}")
            cap = int(old.shape[1]) if cap is None else int(cap)
            if cap < old.shape[1]:
                raise ValueError("cap must not be below the given tree's")
        if explore is None:
            ep, ec = uct_tables(c)
        else:
            try:
                ep, ec = (np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a,
                                               np.float32) for a in explore)
            except (TypeError, ValueError):
                raise ValueError("explore must be two float32 tables (ep, ec)") from None
            if ep.ndim != 1 or ep.shape != ec.shape:
                raise ValueError("explore: ep and ec must be one-dimensional and of the same length")
            if not (np.isfinite(ep).all() and np.isfinite(ec).all()):
                raise ValueError("explore: ep and ec must be finite")
        SparcCore._check_mcts(M, sims, L, 0, len(ep), cap)
        rec = snap.records
        if not isinstance(rec, torch.Tensor):
            rec = torch.from_numpy(np.ascontiguousarray(rec, np.uint8))
        rec = rec.to(dev).contiguous()
        if tree is None:
            nodes = torch.zeros((M, cap, _lib.MCTS_NODE_WORDS), dtype=torch.int32, device=dev)
            count = torch.zeros(M, dtype=torch.int32, device=dev)
            win = torch.zeros((M, rb), dtype=torch.uint8, device=dev)
            wsteps = torch.full((M,), -1, dtype=torch.int32, device=dev)
        else:
            nodes = old.view(torch.int32)
            if cap > nodes.shape[1]:
                grown = torch.zeros((M, cap, _lib.MCTS_NODE_WORDS), dtype=torch.int32, device=dev)
                grown[:, :nodes.shape[1]] = nodes
                nodes = grown
            count, win, wsteps = tree["count"], tree["win"], tree["win_steps"]
            win = win.records if isinstance(win, Snapshot) else win
            if not (isinstance(count, torch.Tensor) and count.dtype == torch.int32 and tuple(count.shape) == (M,) and
                    count.is_contiguous() and count.device == dev):
                raise ValueError(f"tree['count'] must be a contiguous int32 tensor [{M}] on {dev}")
            if not (isinstance(win, torch.Tensor) and win.dtype == torch.uint8 and tuple(win.shape) == (M, rb) and
                    win.is_contiguous() and win.device == dev):
                raise ValueError(f"tree['win'] must hold contiguous uint8 records [{M}, {rb}] on {dev}")
            if not (isinstance(wsteps, torch.Tensor) and tuple(wsteps.shape) == (M,) and
                    not wsteps.dtype.is_floating_point and wsteps.device == dev):
                raise ValueError(f"tree['win_steps'] must be an integer tensor [{M}] on {dev}")
            wsteps = wsteps.to(torch.int32).contiguous()      # -1 is the kernel's 0xFFFFFFFF
        tab = torch.from_numpy(np.stack([ep, ec])).to(dev)    # [2, T]
        status = torch.empty(M, dtype=torch.uint8, device=dev)
        done = torch.empty(M, dtype=torch.int32, device=dev)
        self.core.mcts_device(snap.info, rec.data_ptr(), M, sims, L, tab[0].data_ptr(), tab[1].data_ptr(), len(ep), cap,
                              nodes.data_ptr(), count.data_ptr(), status.data_ptr(), done.data_ptr(), win.data_ptr(),
                              wsteps.data_ptr(), seed=seed, id0=id0,
                              flags=_lib.PLAYOUT_FORWARD if forward_only else 0)
        return {"status": status, "sims": done, "nodes": nodes.view(torch.uint32), "count": count,
                "win": Snapshot(win, snap.info), "win_steps": wsteps.to(torch.int64)}


class SPaRCVecEnv(_RecordReplay, _RecordObserve, _RecordReach, _RecordMcts):
    def __init__(self, num_envs, puzzles=None, df_name="lkaesberg/SPaRC", df_split="all", df_set="test",
                 observation="new", traceback=False, max_steps=2000, autoreset="next_step", device=0,
                 env_offset=0, pitch=None, words=None, processed=None, table=None, rules=False, copy=True,
                 fit_cap=None, rule_table_entries=None):
        if observation not in ("new", "compact"):
            raise ValueError("observation must be 'new' or 'compact' for the vector env")
        self.num_envs = int(num_envs)
        self.observation = observation
        # copy=True (gymnasium's vector-env default): every step() returns observation tensors
        # of its own, so an (obs, next_obs) pair kept by the caller stays intact; copy=False
        # returns the env's buffers, overwritten in place by the next step (the reference's
        # by-reference planes, SPaRC_Gym.py:979)
        self.copy = bool(copy)
        self.traceback = bool(traceback)
        self.max_steps = max_steps
        self.autoreset = autoreset
        self.device = torch.device("cuda", device)
        if processed is None:
            processed = process_puzzles(load_puzzle_source(puzzles, df_name, df_split, df_set))
        self.puzzles = processed
        self.table = table if table is not None else pack_table(processed, pitch, words)
        self.num_puzzles = self.table.num_puzzles
        self.core = SparcCore(self.table, self.num_envs, traceback, max_steps, autoreset, device, env_offset)
        # rule-audit limits (tests force the host fallback of the exact fit with a tiny cap)
        if fit_cap is not None or rule_table_entries is not None:
            self.core.set_rule_limits(fit_cap or 0, rule_table_entries or 0)
        self.x_dim, self.y_dim = self.table.x_max, self.table.y_max
        n, dev = self.num_envs, self.device
        self._act = torch.empty(n, dtype=torch.uint8, device=dev)
        self._rew = torch.empty(n, dtype=torch.int8, device=dev)
        self._flags = torch.empty(n, dtype=torch.uint8, device=dev)
        self._pidx = torch.empty(n, dtype=torch.int32, device=dev)
        self._pos = torch.empty(n, dtype=torch.int32, device=dev)
        self._loc = torch.empty((n, 2), dtype=torch.int32, device=dev)
        if observation == "new":
            self._vis = torch.empty((n, self.x_dim, self.y_dim), dtype=torch.int32, device=dev)
            self._agent = torch.empty_like(self._vis)
            self._build_static()
        self._cursor = np.arange(n, dtype=np.int64) % self.num_puzzles   # "__init__ loads" env i -> i mod P
        self.rules = bool(rules)
        self._rbits = None
        if self.rules:
            self._load_rules()
        self._np_random = None
        self._bound_stream = None

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        s = torch.cuda.current_stream(self.device)
        if self._bound_stream != s.cuda_stream:
            self.core.set_stream(s.cuda_stream)
            self._bound_stream = s.cuda_stream
        return s

    def _build_static(self):
        keys = []
        for p in self.puzzles:
            for k in p["obs_array"]:
                if k not in keys and k not in ("visited", "agent_location"):
                    keys.append(k)
        self.static_keys = keys + ["color", "additional_info"]
        P, X, Y = self.num_puzzles, self.x_dim, self.y_dim
        st = np.zeros((P, len(self.static_keys), X, Y), np.int64)
        for q, p in enumerate(self.puzzles):
            px, py = p["x_size"], p["y_size"]
            for j, k in enumerate(keys):
                if k in p["obs_array"]:
                    st[q, j, :px, :py] = p["obs_array"][k]
            tx, ty = p["target_location"]
            st[q, keys.index("target_location"), :, :] = 0
            st[q, keys.index("target_location"), tx, ty] = 1
            st[q, -2, :px, :py] = p["color_array"]
            st[q, -1, :px, :py] = p["additional_info"]
        self.static_planes = torch.from_numpy(st).to(self.device)

    def _obs(self):
        """Observation of the current state (after reset): separate copy / obs-pack launches."""
        self.core.copy_state_device(4, self._pidx.data_ptr())
        self.core.copy_state_device(1, self._pos.data_ptr())
        if self.observation == "new":
            self.core.obs_pack_device(self._vis.data_ptr(), self._agent.data_ptr(), self.x_dim, self.y_dim)
        return self._obs_dict()

    def _stage_host_actions(self, actions, stream):
        """numpy integer actions -> the device through pinned int64 staging buffers (two, used
        alternately) and an asynchronous copy on the step's stream (torch.as_tensor of a
        pageable array is a synchronous copy; tools/prof_vec_step.py).  A buffer's event,
        recorded on the stream that runs its copy, keeps a later call from overwriting it before
        the copy has read it.  The device copy is a fresh allocation on that stream (the caching
        allocator orders its reuse on the stream), so a caller that switches streams between
        steps cannot overwrite actions a previous step's kernel is still reading."""
        n = self.num_envs
        if getattr(self, "_pin", None) is None:
            self._pin = [torch.empty(n, dtype=torch.int64, pin_memory=True) for _ in range(2)]
            self._pin_done = [None, None]
            self._pin_k = 0
        k = self._pin_k = self._pin_k ^ 1
        if self._pin_done[k] is not None:
            self._pin_done[k].synchronize()
        np.copyto(self._pin[k].numpy(), actions, casting="unsafe")   # integer widening only
        act = torch.empty(n, dtype=torch.int64, device=self.device)
        act.copy_(self._pin[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
        self._pin_done[k] = ev
        return act

    def _step_obs_dict(self, bufs):
        """_obs_dict after step_gym_device, which wrote the agent's (x, y) into loc itself."""
        vis, agent, pidx, loc = bufs
        if self.observation == "compact":
            return {"puzzle_index": pidx, "agent_location": loc}
        return {"visited": vis, "agent_location": agent, "puzzle_index": pidx, "agent_xy": loc}

    def _step_obs_buffers(self):
        """(visited, agent_location, puzzle_index, agent_xy) targets of one step: fresh tensors
        with copy=True, else the env's own buffers."""
        if not self.copy:
            new = self.observation == "new"
            return (self._vis if new else None, self._agent if new else None, self._pidx, self._loc)
        n, dev = self.num_envs, self.device
        vis = agent = None
        if self.observation == "new":
            vis = torch.empty((n, self.x_dim, self.y_dim), dtype=torch.int32, device=dev)
            agent = torch.empty_like(vis)
        return (vis, agent, torch.empty(n, dtype=torch.int32, device=dev),
                torch.empty((n, 2), dtype=torch.int32, device=dev))

    def _obs_dict(self):
        loc = torch.stack([self._pos & 0xFF, (self._pos >> 8) & 0xFF], dim=1)
        pidx = self._pidx.clone() if self.copy else self._pidx
        if self.observation == "compact":
            return {"puzzle_index": pidx, "agent_location": loc}
        if self.copy:
            return {"visited": self._vis.clone(), "agent_location": self._agent.clone(), "puzzle_index": pidx,
                    "agent_xy": loc}
        return {"visited": self._vis, "agent_location": self._agent, "puzzle_index": pidx, "agent_xy": loc}

    def _load_rules(self):
        if self._rbits is None:
            self.core.load_rules(pack_rules(self.puzzles, self.table))
            self._rbits = torch.empty(self.num_envs, dtype=torch.int16, device=self.device)

    def rule_audit(self, region=False, fit=False):
        """The rule audit of every env's current state on the GPU (k_rules): dict with ``bits``
        [N] int16 (bit k = RULE_NAMES[k] passed), optionally ``region`` [N, 64*words] uint8
        (region id per cell bit, the reference's numbering; 255 elsewhere) and ``fit`` [N]
        int64 (bit r: region r passed the poly/ylop area check and exact fit)."""
        self._stream()
        self._load_rules()
        n = self.num_envs
        out = {"bits": self._rbits}
        if region:
            out["region"] = torch.empty((n, 64 * self.table.words), dtype=torch.uint8, device=self.device)
        if fit:
            out["fit"] = torch.empty(n, dtype=torch.int64, device=self.device)
        self.core.rules_device(self._rbits.data_ptr(), out["region"].data_ptr() if region else None,
                               out["fit"].data_ptr() if fit else None)
        # exact fits that passed the GPU's node cap: finished on the host.  This synchronises the
        # stream (a 4-byte read of the queue count when nothing was queued), so rule_audit() and
        # step() with rules=True return final bits and are synchronous
        self.core.rules_finish(self._rbits.data_ptr(), out["fit"].data_ptr() if fit else None)
        return out

    @property
    def np_random(self):
        if self._np_random is None:
            self._np_random = np.random.Generator(np.random.PCG64(np.random.SeedSequence()))
        return self._np_random

    # ------------------------------------------------------------------ API
    def current_puzzle_indices(self):
        """[N] int64: each env's current puzzle index (the reference's current_puzzle_index),
        read from the device, so it follows the device's autoresets.  Before the first
        reset: env i -> i mod P (the vector form of __init__ loading puzzle 0, SPaRC_Gym.py:90)."""
        if not self.core.has_state:
            return self._cursor.copy()
        self._stream()   # the copy below and the read after it run on the caller's current stream
        cur = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        self.core.copy_state_device(4, cur.data_ptr())
        return cur.cpu().numpy().astype(np.int64)

    def reset(self, seed=None, options=None):
        """Per-env puzzle choice as SPaRC_Gym.reset (SPaRC_Gym.py:1075-1087), vectorised:
        * options given: options['puzzle_index'] ([N] ints, this build's extension) or
          options['puzzle_id'] (one id or [N] ids); an env whose id is missing (or any options
          without either key, e.g. {}) keeps its current puzzle (1076-1082);
        * else seed: Generator(PCG64(SeedSequence(seed))).integers(P, size=N) (1084-1085; env
          0 gets the reference's index);
        * else sequential: current index + 1 mod P (1087).
        "Current" is the device's puzzle index, which next-step autoresets advance."""
        self._stream()
        P = self.num_puzzles
        if options is not None and "puzzle_index" in options:
            q = np.asarray(options["puzzle_index"], np.int64)
        elif options is not None:
            cur = self.current_puzzle_indices()
            want = options.get("puzzle_id", None)
            if want is None:
                q = cur
            else:
                ids = {p["id"]: i for i, p in reversed(list(enumerate(self.puzzles)))}
                want = [want] * self.num_envs if isinstance(want, str) or not hasattr(want, "__len__") else list(want)
                if len(want) != self.num_envs:
                    raise ValueError(f"options['puzzle_id'] must be one id or {self.num_envs} ids")
                q = np.array([ids.get(w, c) for w, c in zip(want, cur)], np.int64)
        elif seed is not None:
            self._np_random = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))
            q = self._np_random.integers(P, size=self.num_envs)
        else:
            q = (self.current_puzzle_indices() + 1) % P
        if q.shape != (self.num_envs,) or q.min() < 0 or q.max() >= P:
            raise ValueError("puzzle indices must be [num_envs] in [0, num_puzzles)")
        self._cursor = q.copy()
        flags = self.core.reset_host(q.astype(np.uint32))
        info = {"legal_mask": torch.from_numpy(((flags >> 2) & 0xF).astype(np.uint8)).to(self.device)}
        if self.rules:
            info["rule_bits"] = self.rule_audit()["bits"]
        return self._obs(), info

    def step(self, actions):
        """One step() of every env: actions [N] (uint8: >= 4 is illegal = no move; other integer
        types: < 0 or >= 4 is illegal).  ONE launch (sparc_step_gym_device) writes the step, the
        post-step observation and the gym outputs: reward [N] float64 (the reference's exact
        values), terminated / truncated [N] bool, and info's legal_mask, autoreset and
        reward_code.  Every returned tensor is fresh per call (copy=True, the default); with
        copy=False the observation tensors and reward_code are the env's buffers, overwritten
        by the next step (the reference returns its planes by reference, SPaRC_Gym.py:979)."""
        self._stream()
        n = self.num_envs
        if isinstance(actions, np.ndarray) and actions.shape == (n,) and actions.dtype.kind in "iu":
            a = self._stage_host_actions(actions, torch.cuda.current_stream(self.device))
        else:
            a = torch.as_tensor(actions, device=self.device)
        if a.shape != (n,):
            raise ValueError(f"actions must have shape ({n},)")
        if a.dtype not in (torch.uint8, torch.int32, torch.int64):
            if a.dtype.is_floating_point or a.dtype == torch.bool:
                raise ValueError("actions must be integers")
            a = a.to(torch.int64)
        a = a.contiguous()
        # one allocation for the fresh outputs: reward f64 [N] | terminated | truncated | legal | autoreset
        buf = torch.empty(12 * n, dtype=torch.uint8, device=self.device)
        reward = buf[:8 * n].view(torch.float64)
        terminated = buf[8 * n:9 * n].view(torch.bool)
        truncated = buf[9 * n:10 * n].view(torch.bool)
        legal = buf[10 * n:11 * n]
        autoreset = buf[11 * n:].view(torch.bool)
        new = self.observation == "new"
        bufs = self._step_obs_buffers()
        vis, agent, pidx, loc = bufs
        self.core.step_gym_device(a.data_ptr(), a.element_size(), reward.data_ptr(), terminated.data_ptr(),
                                  truncated.data_ptr(), legal.data_ptr(), autoreset.data_ptr(), self._rew.data_ptr(),
                                  self._flags.data_ptr(), vis.data_ptr() if new else None,
                                  agent.data_ptr() if new else None, self.x_dim if new else 1,
                                  self.y_dim if new else 1, pidx.data_ptr(), loc.data_ptr())
        if self.copy:
            self._loc = loc   # the latest agent (x, y), as the step path wrote it
        info = {"legal_mask": legal, "autoreset": autoreset,
                "reward_code": self._rew.clone() if self.copy else self._rew}
        if self.rules:
            bits = self.rule_audit()["bits"]
            info["rule_bits"] = bits.clone() if self.copy else bits
        return self._step_obs_dict(bufs), reward, terminated, truncated, info

    def rollout(self, T, actions=None, seed=0, t0=0, stats=None, record=True, out=None, obs=False, obs_out=None,
                rules=False):
        """T steps of every env in ONE kernel launch.  actions: [T, N] uint8 on the GPU or None
        (counter-based random actions, sparc_rand_action(seed, env_offset + i, t0 + t)).
        Returns reward codes and flags [T, N] (int8 / uint8) if ``record`` (written into
        ``out=(reward_code, flags)`` when given).  With ``obs`` (or ``obs_out=(visited,
        agent_location)``) the 'new' observation after every step is recorded too: int32
        traces [T, N, x_dim, y_dim] under "visited" / "agent_location" (8 * x_dim * y_dim
        bytes per env-step of HBM writes).  With ``rules`` the rule audit runs after every step
        as in the reference's step() (SPaRC_Gym.py:1227): "rule_bits" [T, N] int16 (bit k =
        RULE_NAMES[k] passed), step t's bits equal rule_audit() after t + 1 single steps."""
        self._stream()
        n = self.num_envs
        if actions is not None:
            actions = torch.as_tensor(actions, device=self.device)
            if actions.shape != (T, n) or actions.dtype != torch.uint8 or not actions.is_contiguous():
                raise ValueError(f"actions must be a contiguous uint8 tensor of shape ({T}, {n})")
        rew = flags = None
        if out is not None:
            rew, flags = out
            for t_, dt in ((rew, torch.int8), (flags, torch.uint8)):
                if t_.shape != (T, n) or t_.dtype != dt or not t_.is_contiguous() or t_.device != self.device:
                    raise ValueError(f"out tensors must be contiguous [{T}, {n}] int8 / uint8 on {self.device}")
        elif record:
            rew = torch.empty((T, n), dtype=torch.int8, device=self.device)
            flags = torch.empty((T, n), dtype=torch.uint8, device=self.device)
        if stats is not None and (stats.shape != (n, 4) or stats.dtype != torch.int32 or not stats.is_contiguous()):
            raise ValueError("stats must be a contiguous int32 tensor [N, 4]")
        args = (None if actions is None else actions.data_ptr(), None if rew is None else rew.data_ptr(),
                None if flags is None else flags.data_ptr(), None if stats is None else stats.data_ptr())
        if rules:
            if obs or obs_out is not None:
                raise ValueError("rules=True records the rule bits only (no observation traces)")
            self._load_rules()
            bits = torch.empty((T, n), dtype=torch.int16, device=self.device)
            self.core.rollout_rules_device(T, *args, bits.data_ptr(), seed, t0)
            self.core.rules_finish(bits.data_ptr())   # searches past the GPU's node cap (a sync)
            return {"reward_code": rew, "flags": flags, "rule_bits": bits}
        if not obs and obs_out is None:
            self.core.rollout_device(T, *args, seed, t0)
            return {"reward_code": rew, "flags": flags}
        X, Y = self.x_dim, self.y_dim
        if obs_out is not None:
            vis, agent = obs_out
            for t_ in (vis, agent):
                if t_ is not None and (t_.shape != (T, n, X, Y) or t_.dtype != torch.int32 or
                                       not t_.is_contiguous() or t_.device != self.device):
                    raise ValueError(f"obs_out tensors must be contiguous int32 [{T}, {n}, {X}, {Y}] on {self.device}")
        else:
            vis = torch.empty((T, n, X, Y), dtype=torch.int32, device=self.device)
            agent = torch.empty_like(vis)
        self.core.rollout_obs_device(T, *args, None if vis is None else vis.data_ptr(),
                                     None if agent is None else agent.data_ptr(), X, Y, seed, t0)
        return {"reward_code": rew, "flags": flags, "visited": vis, "agent_location": agent}

    def random_actions(self, T, seed=0, t0=0, out=None):
        """[T, N] uint8 uniform random actions written on the GPU: ``action_space.sample()``
        (Final_Product.py:29) for every env and step, entry (t, i) = sparc_rand_action(seed,
        env_offset + i, t0 + t) — the actions ``rollout(T, None, seed, t0)`` draws, keyed by the
        global env id (a rank's shard holds the columns of one process over all envs)."""
        self._stream()
        n = self.num_envs
        if out is None:
            out = torch.empty((T, n), dtype=torch.uint8, device=self.device)
        elif out.shape != (T, n) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous uint8 tensor [{T}, {n}] on {self.device}")
        self.core.random_actions_device(T, out.data_ptr(), seed, t0)
        return out

    # ------------------------------------------------------------------ snapshot / restore / fork
    def _index_arg(self, idx, what, limit):
        """An env / record index list for the device: [len] int32 tensor.  A host-side list or
        array is range-checked here (ValueError); a tensor is passed through and checked by the
        kernel (an env with a bad index keeps its state, and the next sync raises)."""
        if isinstance(idx, torch.Tensor):
            if idx.ndim != 1 or idx.dtype.is_floating_point or idx.dtype == torch.bool:
                raise ValueError(f"{what} must be a one-dimensional integer tensor")
            return idx.to(device=self.device, dtype=torch.int32).contiguous()
        a = np.asarray(idx)
        if a.ndim != 1 or a.dtype.kind not in "iu" or a.size == 0:
            raise ValueError(f"{what} must be a non-empty one-dimensional integer array")
        if int(a.min()) < 0 or int(a.max()) >= limit:
            raise ValueError(f"{what} entries must be in [0, {limit})")
        return torch.from_numpy(a.astype(np.int32)).to(self.device)

    def _mask_arg(self, mask):
        if mask is None:
            return None
        if isinstance(mask, torch.Tensor):
            m = mask.to(device=self.device)
        else:
            m = torch.from_numpy(np.asarray(mask)).to(self.device)
        if m.shape != (self.num_envs,):
            raise ValueError(f"mask must have shape ({self.num_envs},)")
        return (m != 0).to(torch.uint8).contiguous()

    def _restored(self, flags, mask):
        """(obs, info) after a restore / fork, as reset() returns them."""
        restored = torch.ones(self.num_envs, dtype=torch.bool, device=self.device) if mask is None else mask.bool()
        info = {"legal_mask": (flags >> 2) & 0xF, "restored": restored}
        if self.rules:
            info["rule_bits"] = self.rule_audit()["bits"]
        return self._obs(), info

    def snapshot(self, envs=None):
        """The state of env ``envs[j]`` (default: every env) as a ``Snapshot`` of opaque records on
        the GPU, everything the step kernels keep per env (the reference's counterpart is a copy
        of the env object, fields SPaRC_Gym.py:141-187).  One launch, asynchronous."""
        from .snapshot import Snapshot
        self._stream()
        info = self.core.snapshot_info()
        idx = None if envs is None else self._index_arg(envs, "envs", self.num_envs)
        M = self.num_envs if idx is None else int(idx.shape[0])
        if M < 1:
            raise ValueError("envs must not be empty")
        rec = torch.empty((M, info.record_bytes), dtype=torch.uint8, device=self.device)
        self.core.snapshot_device(None if idx is None else idx.data_ptr(), M, rec.data_ptr())
        return Snapshot(rec, info)

    def restore(self, snap, src=None, mask=None):
        """Env ``i`` with ``mask[i]`` (default: all) takes record ``src[i]`` of ``snap`` (default:
        record ``i``, which needs ``len(snap) == num_envs``).  Returns ``(obs, info)`` as
        ``reset()``: ``info['legal_mask']`` [N] uint8 (0 for envs not restored),
        ``info['restored']`` the bool mask.  ValueError naming the field when the snapshot's header
        does not match this env (words, pitch, traceback, max_steps, record_bytes, table_hash);
        ``autoreset`` may differ: pending envs of a snapshot then autoreset on their next step."""
        from .snapshot import info_mismatch
        self._stream()
        bad = info_mismatch(snap.info, self.core.snapshot_info())
        if bad is not None:
            raise ValueError(f"snapshot does not match this env: {bad} differs")
        M, n = len(snap), self.num_envs
        if M < 1:
            raise ValueError("empty snapshot")
        if src is None and M != n:
            raise ValueError(f"src is needed to restore {M} records into {n} envs")
        idx = None if src is None else self._index_arg(src, "src", M)
        if idx is not None and idx.shape != (n,):
            raise ValueError(f"src must have shape ({n},)")
        m = self._mask_arg(mask)
        rec = snap.records
        if not isinstance(rec, torch.Tensor):
            rec = torch.from_numpy(np.ascontiguousarray(rec, np.uint8))
        rec = rec.to(self.device).contiguous()
        flags = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self.core.restore_device(snap.info, rec.data_ptr(), M, None if idx is None else idx.data_ptr(),
                                 None if m is None else m.data_ptr(), flags.data_ptr())
        return self._restored(flags, m)

    def fork(self, src, mask=None):
        """Env ``i`` with ``mask[i]`` (default: all) takes the state of env ``src[i]``, as one
        simultaneous assignment (every read sees the state from before the call: permutations
        and fan-out from one env are fine).  Returns ``(obs, info)`` as ``restore``."""
        self._stream()
        n = self.num_envs
        idx = self._index_arg(src, "src", n)
        if idx.shape != (n,):
            raise ValueError(f"src must have shape ({n},)")
        m = self._mask_arg(mask)
        flags = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self.core.fork_device(idx.data_ptr(), None if m is None else m.data_ptr(), flags.data_ptr())
        return self._restored(flags, m)

    def expand(self, snap=None, envs=None):
        """All four successors of every record of ``snap`` (default: ``self.snapshot(envs)``), in
        one launch and without changing any env: the one-ply step of a tree search over a
        frontier of any size.  Returns a dict: ``children`` a ``Snapshot`` of ``4 * M`` records
        on the GPU, child ``(j, a)`` at row ``4 * j + a``, byte for byte what ``restore`` of
        record ``j``, one ``step`` with action ``a`` and ``snapshot`` give under this env's
        ``max_steps`` and ``autoreset`` (an illegal ``a``: the no-move state with step + 1; a
        pending parent under next-step autoreset: four identical reset children, flag 64);
        ``reward_code`` [M, 4] int8 and ``flags`` [M, 4] uint8 of those steps; ``legal_mask`` [M]
        uint8, bits 0-3: the parents' legal actions, as ``info['legal_mask']``.  ValueError
        naming the field when the snapshot's header does not match this env, as ``restore``."""
        from .snapshot import Snapshot, info_mismatch
        self._stream()
        if snap is None:
            snap = self.snapshot(envs)
        elif envs is not None:
            raise ValueError("give snap or envs, not both")
        bad = info_mismatch(snap.info, self.core.snapshot_info())
        if bad is not None:
            raise ValueError(f"snapshot does not match this env: {bad} differs")
        M = len(snap)
        if M < 1 or 4 * M >= 2**31:
            raise ValueError("a snapshot of 1 .. 2^29 - 1 records is needed")
        rec = snap.records
        if not isinstance(rec, torch.Tensor):
            rec = torch.from_numpy(np.ascontiguousarray(rec, np.uint8))
        rec = rec.to(self.device).contiguous()
        children = torch.empty((4 * M, snap.info.record_bytes), dtype=torch.uint8, device=self.device)
        out = torch.empty(9 * M, dtype=torch.uint8, device=self.device)   # codes | flags | parent flags
        code, flags, pflags = out[:4 * M].view(torch.int8).view(M, 4), out[4 * M:8 * M].view(M, 4), out[8 * M:]
        self.core.expand_device(snap.info, rec.data_ptr(), M, children.data_ptr(), code.data_ptr(), flags.data_ptr(),
                                pflags.data_ptr())
        return {"children": Snapshot(children, snap.info), "reward_code": code, "flags": flags,
                "legal_mask": (pflags >> 2) & 0xF}

    def playout(self, snap, playouts, horizon, seed=0, id0=0, forward_only=False, trace=False, final=False,
                stats=True):
        """``playouts`` (K) independent random continuations of every record of ``snap`` (M of
        them), each at most ``horizon`` (L) steps, uniform over the LEGAL actions of each state
        (``search.rand_pick(seed, id0 + j * K + k, t, mask)``), in one launch and without changing
        or reading any env (k_playout).  A playout ends with the step that terminates or
        truncates, never in the next episode, whatever this env's ``autoreset``.
        ``forward_only``: on a traceback env the pop back to the previous point is never drawn; a
        state whose only legal move is the pop ends the playout (a dead end).  Without traceback
        it has no effect.

        Returns a dict of GPU tensors, [M, K] each: ``reward_code`` int8 and ``flags`` uint8 of the
        last step (0 without one), ``steps`` int32 the steps taken,
        ``first`` uint8 the first action (255: none), ``end`` uint8 the end reason (``_lib.END_*``:
        0 bad record, 1 terminated, 2 truncated, 3 horizon, 4 dead end, 5 the record was already
        done), ``return`` int32 the sum of the reward codes; with ``trace`` the actions [L, M, K]
        uint8 (255 at and after the end); with ``final`` a ``Snapshot`` of the M * K end states
        (row ``j * K + k``); with ``stats`` [M, 4, 4] int32, per record and first action
        {playouts, ended with code +100, ended with code -100, steps}.  A record that fails the
        kernel's checks gives end 0 and zeroed outputs, and the next ``core.sync()`` raises.
        ValueError naming the field when the snapshot's header does not match this env."""
        from .snapshot import Snapshot, info_mismatch
        self._stream()
        bad = info_mismatch(snap.info, self.core.snapshot_info())
        if bad is not None:
            raise ValueError(f"snapshot does not match this env: {bad} differs")
        M, K, L = len(snap), int(playouts), int(horizon)
        if M < 1 or K < 1 or M * K >= 2**31:
            raise ValueError("at least one record and one playout, fewer than 2^31 playouts in all, are needed")
        if not 1 <= L <= 65535 or K * L >= 2**31:
            raise ValueError("horizon must be in 1..65535 with playouts * horizon below 2^31")
        rec = snap.records
        if not isinstance(rec, torch.Tensor):
            rec = torch.from_numpy(np.ascontiguousarray(rec, np.uint8))
        rec = rec.to(self.device).contiguous()
        MK = M * K
        dev = self.device
        ret = torch.empty((M, K), dtype=torch.int32, device=dev)
        steps = torch.empty((M, K), dtype=torch.int16, device=dev)
        b = torch.empty((4, M, K), dtype=torch.uint8, device=dev)     # code | flags | first | end
        out = {"reward_code": b[0].view(torch.int8), "flags": b[1], "steps": steps, "first": b[2], "end": b[3],
               "return": ret}
        if trace:
            out["trace"] = torch.empty((L, M, K), dtype=torch.uint8, device=dev)
        fin = torch.empty((MK, snap.info.record_bytes), dtype=torch.uint8, device=dev) if final else None
        if stats:
            out["stats"] = torch.zeros((M, 4, 4), dtype=torch.int32, device=dev)
        self.core.playout_device(snap.info, rec.data_ptr(), M, K, L, seed, id0,
                                 _lib.PLAYOUT_FORWARD if forward_only else 0, d_code=b[0].data_ptr(),
                                 d_flags=b[1].data_ptr(), d_steps=steps.data_ptr(), d_first=b[2].data_ptr(),
                                 d_end=b[3].data_ptr(), d_return=ret.data_ptr(),
                                 d_trace=out["trace"].data_ptr() if trace else None,
                                 d_final=fin.data_ptr() if final else None,
                                 d_stats=out["stats"].data_ptr() if stats else None)
        out["steps"] = steps.to(torch.int32) & 0xFFFF                 # the kernel writes uint16
        if final:
            out["final"] = Snapshot(fin, snap.info)
        return out

    def audit_records(self, snap, region=False, fit=False):
        """The rule audit of every record of ``snap`` (on the host or the GPU, any number of
        them), in one launch and without changing or reading any env (k_rules_rec): what
        ``rule_audit`` gives envs restored from the records.  Returns a dict of GPU tensors:
        ``bits`` [M] int16, optionally ``region`` [M, 64*words] uint8 and ``fit`` [M] int64, with
        ``rule_audit``'s meanings.  Loads the rules on first use; needs no reset.  Exact fits past
        the GPU's node cap are finished on the host, so the bits are final and the call is
        synchronous.  A record that fails the kernel's checks gets bits 0, fit 0 and a region row
        of 255, and the next ``core.sync()`` raises.  ValueError naming the field when the
        snapshot's header does not match this env, as ``restore``."""
        from .snapshot import info_mismatch
        self._stream()
        self._load_rules()
        bad = info_mismatch(snap.info, self.core.snapshot_info())
        if bad is not None:
            raise ValueError(f"snapshot does not match this env: {bad} differs")
        M = len(snap)
        if M < 1 or M >= 2**31:
            raise ValueError("a snapshot of 1 .. 2^31 - 1 records is needed")
        rec = snap.records
        if not isinstance(rec, torch.Tensor):
            rec = torch.from_numpy(np.ascontiguousarray(rec, np.uint8))
        rec = rec.to(self.device).contiguous()
        out = {"bits": torch.empty(M, dtype=torch.int16, device=self.device)}
        if region:
            out["region"] = torch.empty((M, 64 * self.table.words), dtype=torch.uint8, device=self.device)
        if fit:
            out["fit"] = torch.empty(M, dtype=torch.int64, device=self.device)
        d_fit = out["fit"].data_ptr() if fit else None
        self.core.rules_records_device(snap.info, rec.data_ptr(), M, out["bits"].data_ptr(),
                                       out["region"].data_ptr() if region else None, d_fit)
        self.core.rules_finish(out["bits"].data_ptr(), d_fit)   # rec lives until here: the re-run reads it
        return out

    def dfs(self, snap, budget, state=None, counts=None, first=None, undecided=0, prune=False):
        """Depth-first search of the forward-move subtree below every record of ``snap`` (M of
        them), at most ``budget`` entered nodes per record and call, in one launch and without
        changing or reading any env (k_dfs).  A node's children are its legal actions without the
        traceback pop, in action order; a node that reached the target is audited where it stands
        (the audit of ``audit_records``), and only counters, a cursor and a few records come back,
        so the memory does not depend on the tree.  Traceback envs only (ValueError otherwise): the
        record's direction stack is the search stack.  Loads the rules on first use; needs no reset.

        To continue, pass the returned ``cursor`` as ``snap`` together with the returned ``state``,
        ``counts`` and ``first`` (updated in place).  k calls of budget B do exactly the first k * B
        nodes of each record's pre-order walk.

        Returns a dict of GPU tensors / Snapshots: ``status`` [M] uint8 (``_lib.DFS_*``: 0 bad
        record, 1 complete, 2 budget spent, 3 the record was already done, 4 the undecided buffer
        overflowed), ``counts`` [M, 8] int64 accumulated (columns ``_lib.DFS_COUNTER_NAMES``),
        ``cursor`` (Snapshot: where each walk stands; the root again when complete), ``state`` [M]
        int32, ``first`` (Snapshot: the lexicographically least decided satisfying leaf, zeroed where
        none yet), ``found`` and ``done`` [M] bool.  A target leaf whose exact-fit search passed the
        GPU's node cap is *undecided*: counted, not judged.  With ``undecided`` > 0 (the buffer's
        entries) those leaves come back too, to be judged by ``audit_records``: ``undecided``
        (Snapshot of the n stored ones), ``undecided_root`` [n] int64 (their rows of ``snap``) and
        ``undecided_total`` int; a walk whose leaf did not fit stops with status 4 and resumes at
        that leaf.  A record that fails the kernel's checks gets status 0 and a zeroed cursor, and
        the next ``core.sync()`` raises.

        ``prune`` cuts the tree without losing a target leaf.  True or "reach": a node's children are
        only the forward moves through which the free lattice points still connect to the target
        (the ``live`` bits of ``reach`` for that node).  "deadline": of those, only the moves from
        which the target is still reached by ``max_steps`` (step + ``action_dist`` <= max_steps).
        Everything else is the unpruned walk: ``targets``, ``satisfied``, ``listed``, ``both``,
        ``undecided`` and ``first`` are equal, ``nodes`` is smaller, ``dead_ends`` is 0 below the
        root (a root cut off from its target is one dead end) and, under "deadline", ``truncated``
        is 0.  Continue a walk with the ``prune`` it began with: the state word records it, and a
        cursor of another mode is refused like a bad record (status 0).  Any other value raises
        ValueError."""
        from .snapshot import Snapshot, info_mismatch
        mode = _lib.dfs_prune_mode(prune)
        self._stream()
        if not self.traceback:
            raise ValueError("dfs needs a traceback env: the record's direction stack is the search stack")
        bad = info_mismatch(snap.info, self.core.snapshot_info())
        if bad is not None:
            raise ValueError(f"snapshot does not match this env: {bad} differs")
        self._load_rules()
        M, budget, cap = len(snap), int(budget), int(undecided)
        if M < 1 or M >= 2**31:
            raise ValueError("a snapshot of 1 .. 2^31 - 1 records is needed")
        if not 1 <= budget < 2**32:
            raise ValueError("budget must be in 1..2^32-1")
        if cap < 0:
            raise ValueError("undecided must not be negative")
        dev, rb = self.device, snap.info.record_bytes
        rec = snap.records
        if not isinstance(rec, torch.Tensor):
            rec = torch.from_numpy(np.ascontiguousarray(rec, np.uint8))
        rec = rec.to(dev).contiguous()

        def arg(a, shape, dtype, what):
            if a is None:
                return torch.zeros(shape, dtype=dtype, device=dev)
            if isinstance(a, Snapshot):
                a = a.records
            if not (isinstance(a, torch.Tensor) and a.dtype == dtype and tuple(a.shape) == shape and
                    a.is_contiguous() and a.device == dev):
                raise ValueError(f"{what} must be a contiguous {dtype} tensor {list(shape)} on {dev}")
            return a

        state = arg(state, (M,), torch.int32, "state")
        counts = arg(counts, (M, _lib.DFS_COUNTERS), torch.int64, "counts")
        first = arg(first, (M, rb), torch.uint8, "first")
        status = torch.empty(M, dtype=torch.uint8, device=dev)
        cursor = torch.empty((M, rb), dtype=torch.uint8, device=dev)
        und = root = count = None
        if cap:
            und = torch.empty((cap, rb), dtype=torch.uint8, device=dev)
            root = torch.empty(cap, dtype=torch.int32, device=dev)
            count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.core.dfs_device(snap.info, rec.data_ptr(), M, budget, state.data_ptr(), status.data_ptr(),
                             counts.data_ptr(), cursor.data_ptr(), first.data_ptr(),
                             und.data_ptr() if cap else None, root.data_ptr() if cap else None,
                             count.data_ptr() if cap else None, cap, prune=mode)
        out = {"status": status, "counts": counts, "cursor": Snapshot(cursor, snap.info), "state": state,
               "first": Snapshot(first, snap.info), "found": (state & _lib.DFS_STATE_FOUND) != 0,
               "done": (state & _lib.DFS_STATE_DONE) != 0}
        if cap:
            total = int(count.item())
            n = min(total, cap)
            out.update(undecided=Snapshot(und[:n], snap.info), undecided_root=root[:n].to(torch.int64),
                       undecided_total=total)
        return out

    def state(self):
        """Host snapshot of the per-env state (x, y, path_len, step, puzzle, outcome, visited bits)."""
        self._stream()   # read_state copies on the context's stream and synchronises it
        return self.core.read_state()

    def close(self):
        self.core.close()
