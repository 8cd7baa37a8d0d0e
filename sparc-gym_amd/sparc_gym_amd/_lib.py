"""ctypes binding of include/sparc_gym_amd.h (libsparc_gym_amd.so, built for gfx950).

There is no fallback: if the HIP library is missing or fails to load, importing the env
classes raises.  Build it with ``make -C sparc-gym_amd`` (or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsparc_gym_amd.so")   # the in-tree gfx950 build; no override

SPARC_OK = 0
AUTORESET = {"none": 0, "next_step": 1}

c_void_p, c_int32, c_uint64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64


class SparcConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("traceback", ctypes.c_int32), ("max_steps", ctypes.c_int32),
                ("autoreset", ctypes.c_int32), ("pitch", ctypes.c_int32), ("words", ctypes.c_int32),
                ("env_offset", ctypes.c_int64)]


class SparcPuzzleTable(ctypes.Structure):
    _fields_ = [("num_puzzles", ctypes.c_int32), ("num_nodes", ctypes.c_int32),
                ("open", c_void_p), ("info", c_void_p), ("trie", c_void_p)]


class SparcStateHost(ctypes.Structure):
    _fields_ = [("x", c_void_p), ("y", c_void_p), ("path_len", c_void_p), ("step", c_void_p),
                ("puzzle", c_void_p), ("outcome", c_void_p), ("pending", c_void_p), ("visited", c_void_p)]


class SparcRulesTable(ctypes.Structure):
    _fields_ = [("num_puzzles", ctypes.c_int32), ("num_inst", ctypes.c_int32), ("num_shapes", ctypes.c_int32),
                ("num_offsets", ctypes.c_int32), ("planes", c_void_p), ("inst_first", c_void_p), ("inst", c_void_p),
                ("shape_first", c_void_p), ("shape_area", c_void_p), ("shape_off", c_void_p)]


class SparcEnvRecord(ctypes.Structure):
    """sparc_env_record: one env after sparc_env_step / _reset / _read (one round trip)."""
    _fields_ = [("reward_code", ctypes.c_int8), ("flags", ctypes.c_uint8), ("x", ctypes.c_uint8),
                ("y", ctypes.c_uint8), ("path_len", ctypes.c_uint8), ("outcome", ctypes.c_int8),
                ("pending", ctypes.c_uint8), ("audited", ctypes.c_uint8), ("step", ctypes.c_uint32),
                ("puzzle", ctypes.c_uint32), ("rule_bits", ctypes.c_uint16), ("reserved", ctypes.c_uint16),
                ("host_fits", ctypes.c_uint32), ("fit", ctypes.c_uint64), ("visited", ctypes.c_uint64 * 4),
                ("region", ctypes.c_uint8 * 256)]


assert ctypes.sizeof(SparcEnvRecord) == 320

SNAPSHOT_MAGIC = 0x53525053   # SPARC_SNAPSHOT_MAGIC


class SparcSnapshotInfo(ctypes.Structure):
    """sparc_snapshot_info: what the records of a snapshot look like and which table they index."""
    _fields_ = [("magic", ctypes.c_uint32), ("abi_version", ctypes.c_int32), ("words", ctypes.c_int32),
                ("pitch", ctypes.c_int32), ("traceback", ctypes.c_int32), ("max_steps", ctypes.c_int32),
                ("record_bytes", ctypes.c_int32), ("reserved", ctypes.c_int32), ("table_hash", ctypes.c_uint64)]


assert ctypes.sizeof(SparcSnapshotInfo) == 40

PLAYOUT_FORWARD = 1   # SPARC_PLAYOUT_FORWARD
# SPARC_PLAYOUT_END_*: why a playout ended
END_INVALID, END_TERMINATED, END_TRUNCATED, END_HORIZON, END_DEAD_END, END_PENDING = range(6)


class SparcPlayoutOut(ctypes.Structure):
    """sparc_playout_out: the nine outputs of sparc_playout_device / _host, each may be NULL."""
    _fields_ = [(k, c_void_p) for k in ("code", "flags", "steps", "first", "end", "ret", "trace", "final_rec",
                                        "stats")]


REPLAY_STOP_DONE, REPLAY_STOP_ILLEGAL = 1, 2   # SPARC_REPLAY_STOP_*
# SPARC_REPLAY_END_*: why a replayed sequence ended
(REPLAY_END_INVALID, REPLAY_END_TERMINATED, REPLAY_END_TRUNCATED, REPLAY_END_EXHAUSTED, REPLAY_END_ILLEGAL,
 REPLAY_END_PENDING) = range(6)


class SparcReplayOut(ctypes.Structure):
    """sparc_replay_out: the ten outputs of sparc_replay_device / _host, each may be NULL."""
    _fields_ = [(k, c_void_p) for k in ("code", "flags", "steps", "end", "ret", "bad", "step_code", "step_flags",
                                        "final_rec", "states")]


# SPARC_OBS_*: the element type of sparc_observe_records_device's planes
OBS_I32, OBS_U8, OBS_F16, OBS_BF16, OBS_F32 = range(5)
OBS_ELEM_BYTES = {OBS_I32: 4, OBS_U8: 1, OBS_F16: 2, OBS_BF16: 2, OBS_F32: 4}


class SparcObserveOut(ctypes.Structure):
    """sparc_observe_out: the outputs of sparc_observe_records_device / _host, each pointer may be NULL."""
    _fields_ = [("visited", c_void_p), ("agent", c_void_p), ("elem", c_int32), ("x_dim", c_int32),
                ("y_dim", c_int32), ("reserved", c_int32), ("stride", ctypes.c_int64), ("puzzle", c_void_p),
                ("loc", c_void_p), ("legal", c_void_p)]


assert ctypes.sizeof(SparcObserveOut) == 64

# SPARC_REACH_NONE: no way to the target (sparc_reach_records_device's dist and action_dist, its plane's fill)
REACH_NONE = 255


class SparcReachOut(ctypes.Structure):
    """sparc_reach_out: the outputs of sparc_reach_records_device / _host, each pointer may be NULL."""
    _fields_ = [("dist", c_void_p), ("action_dist", c_void_p), ("live", c_void_p), ("size", c_void_p),
                ("plane", c_void_p), ("x_dim", c_int32), ("y_dim", c_int32)]


assert ctypes.sizeof(SparcReachOut) == 48

# SPARC_DFS_*: the status of a record's walk after sparc_dfs_device
DFS_INVALID, DFS_COMPLETE, DFS_BUDGET, DFS_PENDING, DFS_OVERFLOW = range(5)
# the columns of its counters
(DFS_NODES, DFS_TARGETS, DFS_SATISFIED, DFS_LISTED, DFS_BOTH, DFS_DEAD_ENDS, DFS_TRUNCATED, DFS_UNDECIDED,
 DFS_COUNTERS) = range(9)
DFS_COUNTER_NAMES = ("nodes", "targets", "satisfied", "listed", "both", "dead_ends", "truncated", "undecided")
# SPARC_DFS_STATE_*: bits of the state word (bits 0-7: the root's path length, 8-10: the next action)
DFS_STATE_DONE, DFS_STATE_FOUND, DFS_STATE_LEAF, DFS_STATE_STARTED = 1 << 28, 1 << 29, 1 << 30, 1 << 31
# SPARC_DFS_PRUNE_*: the children of a node of sparc_dfs_pruned_device (0: every forward move); the
# state word keeps the mode of its walk in bits 12-13
DFS_PRUNE_REACH, DFS_PRUNE_DEADLINE, DFS_STATE_MODE_SHIFT = 1, 2, 12


def dfs_prune_mode(prune):
    """The ``prune`` argument of ``dfs`` as the C value: False -> 0, True or "reach" -> 1 (only moves
    through which the target can still be reached), "deadline" -> 3 (and reached before max_steps)."""
    if prune is False:
        return 0
    if prune is True or prune == "reach":
        return DFS_PRUNE_REACH
    if prune == "deadline":
        return DFS_PRUNE_REACH | DFS_PRUNE_DEADLINE
    raise ValueError(f'prune must be False, True, "reach" or "deadline", not {prune!r}')


class SparcDfsOut(ctypes.Structure):
    """sparc_dfs_out: the outputs of sparc_dfs_device / _host."""
    _fields_ = [(k, c_void_p) for k in ("status", "counts", "cursor", "first_sat", "und_rec", "und_root",
                                        "und_count")] + [("und_cap", c_uint64)]


# SPARC_MCTS_*: the status of a root's tree after sparc_mcts_device
MCTS_INVALID, MCTS_DONE, MCTS_FULL, MCTS_PENDING, MCTS_DEAD_END = range(5)
MCTS_NODE_WORDS = 16            # SPARC_MCTS_NODE_BYTES / 4: a node is 16 uint32
MCTS_NO_CHILD = 0xFFFFFFFF      # SPARC_MCTS_NO_CHILD: child[a] of an action that is not a child
MCTS_MAX_CAP = 1 << 24          # the largest arena per root, in nodes
# the words of a node: w0 parent | action << 28 | kind << 30, then visits, wins, losses, child[4], n[4], wins[4]
MCTS_VISITS, MCTS_WINS, MCTS_LOSSES, MCTS_CHILD, MCTS_N, MCTS_CHILD_WINS = 1, 2, 3, 4, 8, 12
MCTS_KIND_INNER, MCTS_KIND_TERMINATED, MCTS_KIND_TRUNCATED, MCTS_KIND_DEAD_END = range(4)


class SparcMctsOut(ctypes.Structure):
    """sparc_mcts_out: the outputs of sparc_mcts_device / _host, all needed."""
    _fields_ = [(k, c_void_p) for k in ("status", "sims_done", "win_rec", "win_steps")]


_MCTS_ARGS = [c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64, c_int32, c_int32, c_uint64,
              c_uint64, ctypes.c_uint32, c_void_p, c_void_p, c_int32, ctypes.c_int64, c_void_p, c_void_p,
              ctypes.POINTER(SparcMctsOut)]

_SIGS = {
    "sparc_abi_version": ([], c_int32),
    "sparc_last_error": ([c_void_p], ctypes.c_char_p),
    "sparc_create": ([ctypes.c_int, ctypes.POINTER(SparcConfig), ctypes.POINTER(c_void_p)], c_int32),
    "sparc_destroy": ([c_void_p], c_int32),
    "sparc_set_stream": ([c_void_p, c_void_p], c_int32),
    "sparc_use_own_stream": ([c_void_p], c_int32),
    "sparc_sync": ([c_void_p], c_int32),
    "sparc_load_puzzles": ([c_void_p, ctypes.POINTER(SparcPuzzleTable)], c_int32),
    "sparc_reset_host": ([c_void_p, c_void_p, c_void_p, c_void_p], c_int32),
    "sparc_reset_device": ([c_void_p, c_void_p, c_void_p, c_void_p], c_int32),
    "sparc_step_device": ([c_void_p, c_void_p, c_void_p, c_void_p], c_int32),
    "sparc_step_host": ([c_void_p, c_void_p, c_void_p, c_void_p], c_int32),
    "sparc_rollout_device": ([c_void_p, c_int32, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p],
                             c_int32),
    "sparc_random_actions_device": ([c_void_p, c_int32, c_uint64, c_uint64, c_void_p], c_int32),
    "sparc_obs_pack_device": ([c_void_p, c_void_p, c_void_p, c_int32, c_int32], c_int32),
    "sparc_step_obs_device": ([c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                               c_void_p, c_void_p], c_int32),
    "sparc_step_gym_device": ([c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p],
                              c_int32),
    "sparc_rollout_obs_device": ([c_void_p, c_int32, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_int32, c_int32], c_int32),
    "sparc_rollout_rules_device": ([c_void_p, c_int32, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p,
                                    c_void_p], c_int32),
    "sparc_read_state": ([c_void_p, ctypes.POINTER(SparcStateHost)], c_int32),
    "sparc_env_step": ([c_void_p, c_int32, c_int32, c_int32, ctypes.POINTER(SparcEnvRecord)], c_int32),
    "sparc_env_reset": ([c_void_p, c_int32, ctypes.c_uint32, c_int32, ctypes.POINTER(SparcEnvRecord)], c_int32),
    "sparc_env_read": ([c_void_p, c_int32, c_int32, ctypes.POINTER(SparcEnvRecord)], c_int32),
    "sparc_state_ptr": ([c_void_p, c_int32, ctypes.POINTER(c_void_p)], c_int32),
    "sparc_set_visited_host": ([c_void_p, c_void_p], c_int32),
    "sparc_copy_state_device": ([c_void_p, c_int32, c_void_p], c_int32),
    "sparc_snapshot_info_get": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo)], c_int32),
    "sparc_snapshot_device": ([c_void_p, c_void_p, ctypes.c_int64, c_void_p], c_int32),
    "sparc_restore_device": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64, c_void_p,
                              c_void_p, c_void_p], c_int32),
    "sparc_fork_device": ([c_void_p, c_void_p, c_void_p, c_void_p], c_int32),
    "sparc_snapshot_host": ([c_void_p, c_void_p, ctypes.c_int64, c_void_p], c_int32),
    "sparc_restore_host": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64, c_void_p,
                            c_void_p, c_void_p], c_int32),
    "sparc_expand_device": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64, c_void_p,
                             c_void_p, c_void_p, c_void_p], c_int32),
    "sparc_expand_host": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64, c_void_p,
                           c_void_p, c_void_p, c_void_p], c_int32),
    "sparc_playout_device": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64, c_int32, c_int32,
                              c_uint64, c_uint64, ctypes.c_uint32, ctypes.POINTER(SparcPlayoutOut)], c_int32),
    "sparc_playout_host": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64, c_int32, c_int32,
                            c_uint64, c_uint64, ctypes.c_uint32, ctypes.POINTER(SparcPlayoutOut)], c_int32),
    "sparc_replay_device": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, c_void_p, ctypes.c_int64, c_int32,
                             c_void_p, c_void_p, ctypes.c_uint32, ctypes.POINTER(SparcReplayOut)], c_int32),
    "sparc_replay_host": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, c_void_p, ctypes.c_int64, c_int32,
                           c_void_p, c_void_p, ctypes.c_uint32, ctypes.POINTER(SparcReplayOut)], c_int32),
    "sparc_observe_records_device": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64,
                                      ctypes.POINTER(SparcObserveOut)], c_int32),
    "sparc_observe_records_host": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64,
                                    ctypes.POINTER(SparcObserveOut)], c_int32),
    "sparc_reach_records_device": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64,
                                    ctypes.POINTER(SparcReachOut)], c_int32),
    "sparc_reach_records_host": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64,
                                  ctypes.POINTER(SparcReachOut)], c_int32),
    "sparc_dfs_device": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64, ctypes.c_uint32,
                          c_void_p, ctypes.POINTER(SparcDfsOut)], c_int32),
    "sparc_dfs_host": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64, ctypes.c_uint32,
                        c_void_p, ctypes.POINTER(SparcDfsOut)], c_int32),
    "sparc_dfs_pruned_device": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64,
                                 ctypes.c_uint32, c_int32, c_void_p, ctypes.POINTER(SparcDfsOut)], c_int32),
    "sparc_dfs_pruned_host": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64,
                               ctypes.c_uint32, c_int32, c_void_p, ctypes.POINTER(SparcDfsOut)], c_int32),
    "sparc_mcts_device": (_MCTS_ARGS, c_int32),
    "sparc_mcts_host": (_MCTS_ARGS, c_int32),
    "sparc_load_rules": ([c_void_p, ctypes.POINTER(SparcRulesTable)], c_int32),
    "sparc_rules_device": ([c_void_p, c_void_p, c_void_p, c_void_p], c_int32),
    "sparc_rules_host": ([c_void_p, c_void_p, c_void_p, c_void_p], c_int32),
    "sparc_rules_records_device": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64, c_void_p,
                                    c_void_p, c_void_p], c_int32),
    "sparc_rules_records_host": ([c_void_p, ctypes.POINTER(SparcSnapshotInfo), c_void_p, ctypes.c_int64, c_void_p,
                                  c_void_p, c_void_p], c_int32),
    "sparc_rules_finish": ([c_void_p, c_void_p, c_void_p], c_int32),
    "sparc_set_rule_limits": ([c_void_p, ctypes.c_uint32, c_uint64], c_int32),
    "sparc_set_variant": ([c_void_p, c_int32, c_int32], c_int32),
    "sparc_rules_queue_stats": ([c_void_p, c_void_p], c_int32),
    "sparc_comm_unique_id": ([c_void_p], c_int32),
    "sparc_comm_init": ([c_void_p, c_int32, c_int32, c_void_p, ctypes.POINTER(c_void_p)], c_int32),
    "sparc_comm_destroy": ([c_void_p], c_int32),
    "sparc_gather_stats": ([c_void_p, c_void_p, c_void_p, c_void_p], c_int32),
}
COMM_ID_BYTES = 128   # SPARC_COMM_ID_BYTES
EXPORTS = tuple(_SIGS)

_lib = None


class SparcError(RuntimeError):
    pass


def load(path=None, any_abi=False):
    """Load and type the HIP library (cached).  Raises if it is missing: no CPU fallback.

    The product path always loads the in-tree build (``path=None``).  Profiling tools may load
    another build by calling ``load(path)`` themselves before any env is created; later
    ``load()`` calls then return that library.  ``any_abi``: an A/B build of an earlier ABI
    version (the rollout entry points are unchanged; symbols it lacks stay unbound)."""
    global _lib
    if _lib is not None:
        if path is not None and os.path.abspath(path) != _lib._sparc_path:
            raise ImportError(f"libsparc_gym_amd already loaded from {_lib._sparc_path}")
        return _lib
    path = LIB_PATH if path is None else path
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: build the HIP extension (make -C sparc-gym_amd)")
    lib = ctypes.CDLL(path)
    for name, (args, res) in _SIGS.items():
        if any_abi and not hasattr(lib, name):
            continue
        f = getattr(lib, name)
        f.argtypes = args
        f.restype = res
    if lib.sparc_abi_version() != 2 and not any_abi:
        raise ImportError("libsparc_gym_amd ABI version mismatch")
    lib._sparc_path = os.path.abspath(path)
    _lib = lib
    return lib


def check(rc, ctx=None):
    if rc != SPARC_OK:
        msg = load().sparc_last_error(ctx)
        msg = msg.decode() if msg else "unknown error"
        if rc == -1:
            raise ValueError(msg)
        raise SparcError(f"sparc error {rc}: {msg}")
