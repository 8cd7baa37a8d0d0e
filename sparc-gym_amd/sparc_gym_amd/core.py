"""SparcCore: owns one C-ABI context (one GPU, one batch of envs) and its calls.

Thin, typed wrapper over include/sparc_gym_amd.h used by SPaRCVecEnv (batched) and SPaRC_Gym
(batch of one).  Device pointers are plain ints (e.g. torch ``tensor.data_ptr()``).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .puzzles import PuzzleTable, RulesTable

INT32_MAX = 2**31 - 1


def _ptr(a):
    return None if a is None else a.ctypes.data


class SparcCore:
    def __init__(self, table: PuzzleTable, num_envs: int, traceback=False, max_steps=2000,
                 autoreset="none", device=0, env_offset=0):
        self.lib = _lib.load()
        if autoreset not in _lib.AUTORESET:
            raise ValueError(f"autoreset must be one of {sorted(_lib.AUTORESET)}")
        self.table = table
        self.num_envs = int(num_envs)
        self.traceback = bool(traceback)
        self.max_steps = int(max(min(int(max_steps), INT32_MAX), -INT32_MAX - 1))
        self.device = int(device)
        cfg = _lib.SparcConfig(self.num_envs, int(self.traceback), self.max_steps, _lib.AUTORESET[autoreset],
                               table.pitch, table.words, int(env_offset))
        ctx = ctypes.c_void_p()
        _lib.check(self.lib.sparc_create(self.device, ctypes.byref(cfg), ctypes.byref(ctx)))
        self.ctx = ctx
        self.load_table(table)

    # ---------------------------------------------------------------- lifecycle
    def load_table(self, table: PuzzleTable):
        open_ = np.ascontiguousarray(table.open, np.uint64)
        info = np.ascontiguousarray(table.info, np.uint32)
        trie = np.ascontiguousarray(table.trie, np.uint32)
        t = _lib.SparcPuzzleTable(len(info), len(trie), open_.ctypes.data, info.ctypes.data,
                                  trie.ctypes.data if len(trie) else None)
        self._check(self.lib.sparc_load_puzzles(self.ctx, ctypes.byref(t)))
        self.table = table
        self.has_state = False   # as the context: the old state may name puzzles that are gone

    def load_rules(self, rt: RulesTable):
        """Upload the rule-audit table (puzzles.pack_rules) for the loaded puzzles."""
        planes = np.ascontiguousarray(rt.planes, np.uint64)
        first = np.ascontiguousarray(rt.inst_first, np.uint32)
        inst = np.ascontiguousarray(rt.inst, np.uint32)
        sf = np.ascontiguousarray(rt.shape_first, np.uint32)
        sa = np.ascontiguousarray(rt.shape_area, np.int32)
        so = np.ascontiguousarray(rt.shape_off, np.int8)
        t = _lib.SparcRulesTable(len(first) - 1, len(inst), len(sa), len(so), planes.ctypes.data, first.ctypes.data,
                                 inst.ctypes.data if len(inst) else None, sf.ctypes.data,
                                 sa.ctypes.data if len(sa) else None, so.ctypes.data if len(so) else None)
        self._check(self.lib.sparc_load_rules(self.ctx, ctypes.byref(t)))
        self.rules = rt

    def rules_host(self, region=False, fit=False):
        """Rule audit of every env's current state: dict of bits [N] uint16 (+ region
        [N][64*words] uint8, fit [N] uint64 when asked)."""
        n, W = self.num_envs, self.table.words
        out = {"bits": np.empty(n, np.uint16)}
        if region:
            out["region"] = np.empty((n, 64 * W), np.uint8)
        if fit:
            out["fit"] = np.empty(n, np.uint64)
        self._check(self.lib.sparc_rules_host(self.ctx, _ptr(out["bits"]), _ptr(out.get("region")),
                                              _ptr(out.get("fit"))))
        return out

    def rules_device(self, d_bits, d_region=None, d_fit=None):
        self._check(self.lib.sparc_rules_device(self.ctx, d_bits, d_region, d_fit))

    def rules_records_device(self, info, d_records, M, d_bits, d_region=None, d_fit=None):
        """sparc_rules_records_device: the rule audit of M records (bits [M], region [M][64*words],
        fit [M]); reads the context's tables only (asynchronous; then rules_finish)."""
        self._check(self.lib.sparc_rules_records_device(self.ctx, ctypes.byref(info), d_records, int(M), d_bits,
                                                        d_region, d_fit))

    def rules_records_host(self, info, records, region=False, fit=False):
        """Audit host records [M, record_bytes]: dict of bits [M] uint16 (+ region [M][64*words]
        uint8, fit [M] uint64 when asked), final (synchronous)."""
        rec = np.ascontiguousarray(records, np.uint8)
        if rec.ndim != 2 or rec.shape[1] != info.record_bytes or len(rec) < 1:
            raise ValueError(f"records must be [M, {info.record_bytes}] uint8 with M >= 1")
        M, W = len(rec), self.table.words
        out = {"bits": np.empty(M, np.uint16)}
        if region:
            out["region"] = np.empty((M, 64 * W), np.uint8)
        if fit:
            out["fit"] = np.empty(M, np.uint64)
        self._check(self.lib.sparc_rules_records_host(self.ctx, ctypes.byref(info), _ptr(rec), M, _ptr(out["bits"]),
                                                      _ptr(out.get("region")), _ptr(out.get("fit"))))
        return out

    def rules_finish(self, d_bits, d_fit=None):
        """Finish, on the host and without a node cap, the exact-fit searches of the last audit
        call that passed the GPU's cap, and patch its bits (and fit) in place (synchronous)."""
        self._check(self.lib.sparc_rules_finish(self.ctx, d_bits, d_fit))

    def rules_queue_stats(self):
        """The exact-fit queue: capacity, searches the last rules_finish ran on the host, calls
        run again after a queue overflow."""
        out = np.zeros(3, np.uint64)
        self._check(self.lib.sparc_rules_queue_stats(self.ctx, out.ctypes.data))
        return {"capacity": int(out[0]), "last_searches": int(out[1]), "reruns": int(out[2])}

    def set_rule_limits(self, fit_cap=0, table_entries=0):
        """GPU node cap of one exact-fit search (0: 2^26) and the region-code table budget in
        entries (0: 2^28); the budget applies at the next load_rules."""
        self._check(self.lib.sparc_set_rule_limits(self.ctx, int(fit_cap or 0), int(table_entries or 0)))

    # sparc_set_variant (include/sparc_gym_amd.h): kernel variants with identical results
    VARIANT_IO_CODES_OFF, VARIANT_RULE_ROLLOUT_GENERIC, VARIANT_R1R_SHAPE, VARIANT_OBS_INLINE = 1, 2, 3, 4
    VARIANT_MIXED_TRIE, VARIANT_HOST_FITS = 5, 6

    def set_variant(self, which, value):
        """Debug: select a kernel variant of identical results for this context (A/B, tests)."""
        self._check(self.lib.sparc_set_variant(self.ctx, int(which), int(value)))

    def close(self):
        if getattr(self, "ctx", None) is not None and self.ctx.value:
            self.lib.sparc_destroy(self.ctx)
        self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _check(self, rc):
        _lib.check(rc, self.ctx)

    def set_stream(self, stream_handle):
        """Order all calls on this HIP stream (int handle; 0 = the null stream, e.g. torch's
        default stream)."""
        self._check(self.lib.sparc_set_stream(self.ctx, stream_handle or None))

    def use_own_stream(self):
        self._check(self.lib.sparc_use_own_stream(self.ctx))

    def sync(self):
        self._check(self.lib.sparc_sync(self.ctx))

    # ---------------------------------------------------------------- host-pointer calls
    def reset_host(self, puzzle_index, mask=None):
        q = np.ascontiguousarray(puzzle_index, np.uint32)
        if q.shape != (self.num_envs,):
            raise ValueError(f"puzzle_index must have shape ({self.num_envs},)")
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        if m is not None and m.shape != (self.num_envs,):
            raise ValueError("mask shape mismatch")
        flags = np.zeros(self.num_envs, np.uint8)
        self._check(self.lib.sparc_reset_host(self.ctx, _ptr(q), _ptr(m), _ptr(flags)))
        self.has_state = True
        return flags

    def step_host(self, actions):
        a = np.ascontiguousarray(actions, np.uint8)
        if a.shape != (self.num_envs,):
            raise ValueError(f"actions must have shape ({self.num_envs},)")
        rew = np.empty(self.num_envs, np.int8)
        flags = np.empty(self.num_envs, np.uint8)
        self._check(self.lib.sparc_step_host(self.ctx, _ptr(a), _ptr(rew), _ptr(flags)))
        return rew, flags

    def read_state(self):
        n, W = self.num_envs, self.table.words
        out = {"x": np.empty(n, np.uint8), "y": np.empty(n, np.uint8), "path_len": np.empty(n, np.uint16),
               "step": np.empty(n, np.uint32), "puzzle": np.empty(n, np.uint32), "outcome": np.empty(n, np.int8),
               "pending": np.empty(n, np.uint8), "visited": np.empty((W, n), np.uint64)}
        s = _lib.SparcStateHost(*(out[k].ctypes.data for k in
                                  ("x", "y", "path_len", "step", "puzzle", "outcome", "pending", "visited")))
        self._check(self.lib.sparc_read_state(self.ctx, ctypes.byref(s)))
        return out

    # ---------------------------------------------------------------- one env, one round trip
    def env_step(self, action, audit=False, env=0):
        """sparc_env_step: step env `env` and return its record (state, reward code, flags and,
        with ``audit``, the rule audit of the new state) after ONE stream synchronisation."""
        rec = self._rec()
        self._check(self.lib.sparc_env_step(self.ctx, int(env), int(action), int(bool(audit)), ctypes.byref(rec)))
        return rec

    def env_reset(self, puzzle_index, audit=False, env=0):
        rec = self._rec()
        self._check(self.lib.sparc_env_reset(self.ctx, int(env), int(puzzle_index), int(bool(audit)),
                                             ctypes.byref(rec)))
        self.has_state = True
        return rec

    def env_read(self, audit=False, env=0):
        rec = self._rec()
        self._check(self.lib.sparc_env_read(self.ctx, int(env), int(bool(audit)), ctypes.byref(rec)))
        return rec

    def _rec(self):
        # a fresh record per call: a caller may keep the previous one
        return _lib.SparcEnvRecord()

    def set_visited_host(self, words):
        """Overwrite the visited boards [words][N] uint64 of the current state."""
        v = np.ascontiguousarray(words, np.uint64)
        if v.shape != (self.table.words, self.num_envs):
            raise ValueError(f"visited must have shape ({self.table.words}, {self.num_envs})")
        self._check(self.lib.sparc_set_visited_host(self.ctx, _ptr(v)))

    # ---------------------------------------------------------------- device-pointer calls (async)
    def reset_device(self, d_puzzle_index, d_mask=None, d_flags=None):
        self._check(self.lib.sparc_reset_device(self.ctx, d_puzzle_index, d_mask, d_flags))
        self.has_state = True

    def step_device(self, d_actions, d_reward, d_flags):
        self._check(self.lib.sparc_step_device(self.ctx, d_actions, d_reward, d_flags))

    def rollout_device(self, T, d_actions, d_reward, d_flags, d_stats=None, seed=0, t0=0):
        self._check(self.lib.sparc_rollout_device(self.ctx, int(T), d_actions, int(seed) & (2**64 - 1),
                                                  int(t0), d_reward, d_flags, d_stats))

    def random_actions_device(self, T, d_actions, seed=0, t0=0):
        """[T, N] uint8 counter-based random actions (global env ids) into device memory."""
        self._check(self.lib.sparc_random_actions_device(self.ctx, int(T), int(seed) & (2**64 - 1), int(t0),
                                                         d_actions))

    def step_obs_device(self, d_actions, d_reward, d_flags, d_visited, d_agent, x_dim, y_dim, d_puzzle=None,
                        d_xy=None):
        self._check(self.lib.sparc_step_obs_device(self.ctx, d_actions, d_reward, d_flags, d_visited, d_agent,
                                                   int(x_dim), int(y_dim), d_puzzle, d_xy))

    def step_gym_device(self, d_actions, action_bytes, d_reward=None, d_terminated=None, d_truncated=None,
                        d_legal=None, d_autoreset=None, d_reward_code=None, d_flags=None, d_visited=None,
                        d_agent=None, x_dim=1, y_dim=1, d_puzzle=None, d_loc=None):
        self._check(self.lib.sparc_step_gym_device(self.ctx, d_actions, int(action_bytes), d_reward, d_terminated,
                                                   d_truncated, d_legal, d_autoreset, d_reward_code, d_flags,
                                                   d_visited, d_agent, int(x_dim), int(y_dim), d_puzzle, d_loc))

    def rollout_obs_device(self, T, d_actions, d_reward, d_flags, d_stats, d_visited, d_agent, x_dim, y_dim,
                           seed=0, t0=0):
        self._check(self.lib.sparc_rollout_obs_device(self.ctx, int(T), d_actions, int(seed) & (2**64 - 1),
                                                      int(t0), d_reward, d_flags, d_stats, d_visited, d_agent,
                                                      int(x_dim), int(y_dim)))

    def rollout_rules_device(self, T, d_actions, d_reward, d_flags, d_stats, d_rule_bits, seed=0, t0=0):
        self._check(self.lib.sparc_rollout_rules_device(self.ctx, int(T), d_actions, int(seed) & (2**64 - 1),
                                                        int(t0), d_reward, d_flags, d_stats, d_rule_bits))

    def copy_state_device(self, which, d_out):
        self._check(self.lib.sparc_copy_state_device(self.ctx, int(which), d_out))

    def obs_pack_device(self, d_visited, d_agent, x_dim, y_dim):
        self._check(self.lib.sparc_obs_pack_device(self.ctx, d_visited, d_agent, int(x_dim), int(y_dim)))

    # ---------------------------------------------------------------- snapshot / restore / fork
    def snapshot_info(self):
        """sparc_snapshot_info of this context: record size, shape and the loaded table's hash."""
        info = _lib.SparcSnapshotInfo()
        self._check(self.lib.sparc_snapshot_info_get(self.ctx, ctypes.byref(info)))
        return info

    def snapshot_device(self, d_env, M, d_records):
        self._check(self.lib.sparc_snapshot_device(self.ctx, d_env, int(M), d_records))

    def restore_device(self, info, d_records, M, d_src=None, d_mask=None, d_flags=None):
        self._check(self.lib.sparc_restore_device(self.ctx, ctypes.byref(info), d_records, int(M), d_src, d_mask,
                                                  d_flags))
        self.has_state = True

    def fork_device(self, d_src, d_mask=None, d_flags=None):
        self._check(self.lib.sparc_fork_device(self.ctx, d_src, d_mask, d_flags))

    def snapshot_host(self, envs=None):
        """Records [M, record_bytes] uint8 on the host: of env envs[j], or of every env."""
        e = None if envs is None else np.ascontiguousarray(envs, np.uint32)
        if e is not None and e.ndim != 1:
            raise ValueError("envs must be one-dimensional")
        M = self.num_envs if e is None else len(e)
        rec = np.empty((M, self.snapshot_info().record_bytes), np.uint8)
        self._check(self.lib.sparc_snapshot_host(self.ctx, _ptr(e), M, _ptr(rec)))
        return rec

    def restore_host(self, info, records, src=None, mask=None):
        """Restore host records; returns the flags [N] uint8 (legal actions << 2, 0 if not restored)."""
        rec = np.ascontiguousarray(records, np.uint8)
        s = None if src is None else np.ascontiguousarray(src, np.uint32)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        for a, what in ((s, "src"), (m, "mask")):
            if a is not None and a.shape != (self.num_envs,):
                raise ValueError(f"{what} must have shape ({self.num_envs},)")
        flags = np.zeros(self.num_envs, np.uint8)
        self._check(self.lib.sparc_restore_host(self.ctx, ctypes.byref(info), _ptr(rec), len(rec), _ptr(s), _ptr(m),
                                                _ptr(flags)))
        self.has_state = True
        return flags

    # ---------------------------------------------------------------- one-ply expansion of records
    def expand_device(self, info, d_records, M, d_children, d_reward=None, d_flags=None, d_parent_flags=None):
        """sparc_expand_device: children [M][4] records, reward codes / flags [M][4], the parents'
        legal actions << 2 [M]; reads the context's tables only (asynchronous)."""
        self._check(self.lib.sparc_expand_device(self.ctx, ctypes.byref(info), d_records, int(M), d_children,
                                                 d_reward, d_flags, d_parent_flags))

    def expand_host(self, info, records):
        """Expand host records [M, record_bytes]: (children [4M, record_bytes] uint8, reward codes
        [M, 4] int8, flags [M, 4] uint8, parent flags [M] uint8) on the host (synchronous)."""
        rec = np.ascontiguousarray(records, np.uint8)
        if rec.ndim != 2 or rec.shape[1] != info.record_bytes or len(rec) < 1:
            raise ValueError(f"records must be [M, {info.record_bytes}] uint8 with M >= 1")
        M = len(rec)
        children = np.empty((4 * M, rec.shape[1]), np.uint8)
        rew, flags, pflags = np.empty((M, 4), np.int8), np.empty((M, 4), np.uint8), np.empty(M, np.uint8)
        self._check(self.lib.sparc_expand_host(self.ctx, ctypes.byref(info), _ptr(rec), M, _ptr(children), _ptr(rew),
                                               _ptr(flags), _ptr(pflags)))
        return children, rew, flags, pflags

    # ---------------------------------------------------------------- observation planes of records
    def _check_observe(self, M, elem, x_dim, y_dim, stride, outputs):
        """The argument rules of sparc_observe_records_device that need no device (ValueError)."""
        if elem not in _lib.OBS_ELEM_BYTES:
            raise ValueError("elem must be one of the OBS_* element types")
        if not 1 <= M < 2**31:
            raise ValueError("M must be in 1..2^31-1")
        if x_dim < self.table.x_max or y_dim < self.table.y_max or x_dim * y_dim > 256:
            raise ValueError(f"x_dim, y_dim must be at least {self.table.x_max}, {self.table.y_max} (the table's "
                             "largest lattice) with x_dim * y_dim <= 256")
        if stride < 0 or 0 < stride < x_dim * y_dim:
            raise ValueError("stride must be 0 (dense) or at least x_dim * y_dim")
        if all(x is None for x in outputs):
            raise ValueError("out: at least one output is needed")

    def observe_records_device(self, info, d_records, M, elem=_lib.OBS_I32, x_dim=None, y_dim=None, stride=0,
                               d_visited=None, d_agent=None, d_puzzle=None, d_loc=None, d_legal=None):
        """sparc_observe_records_device: the visited / agent_location planes of M records
        ([x_dim][y_dim] elements of type ``elem``, ``stride`` elements apart, 0: dense), the puzzle
        index [M] uint32, the agent's (x, y) [M][2] int32 and the legal actions [M] uint8, each may
        be None; reads the context's tables only (asynchronous)."""
        M, elem, stride = int(M), int(elem), int(stride)
        x_dim = self.table.x_max if x_dim is None else int(x_dim)
        y_dim = self.table.y_max if y_dim is None else int(y_dim)
        self._check_observe(M, elem, x_dim, y_dim, stride, (d_visited, d_agent, d_puzzle, d_loc, d_legal))
        out = _lib.SparcObserveOut(d_visited, d_agent, elem, x_dim, y_dim, 0, stride, d_puzzle, d_loc, d_legal)
        self._check(self.lib.sparc_observe_records_device(self.ctx, ctypes.byref(info), d_records, M,
                                                          ctypes.byref(out)))

    def observe_records_host(self, info, records, elem=_lib.OBS_I32, x_dim=None, y_dim=None):
        """Observe host records [M, record_bytes]: a dict of host arrays ``visited`` and ``agent``
        [M, x_dim, y_dim] (the element's bytes as uint8 / uint16 / uint32 for 1 / 2 / 4-byte
        elements; int32 for OBS_I32), ``puzzle`` [M] uint32, ``loc`` [M, 2] int32 and ``legal`` [M]
        uint8 (synchronous)."""
        rec = np.ascontiguousarray(records, np.uint8)
        if rec.ndim != 2 or rec.shape[1] != info.record_bytes or len(rec) < 1:
            raise ValueError(f"records must be [M, {info.record_bytes}] uint8 with M >= 1")
        M, elem = len(rec), int(elem)
        x_dim = self.table.x_max if x_dim is None else int(x_dim)
        y_dim = self.table.y_max if y_dim is None else int(y_dim)
        self._check_observe(M, elem, x_dim, y_dim, 0, (True,))
        dt = np.int32 if elem == _lib.OBS_I32 else {1: np.uint8, 2: np.uint16, 4: np.uint32}[_lib.OBS_ELEM_BYTES[elem]]
        out = {"visited": np.empty((M, x_dim, y_dim), dt), "agent": np.empty((M, x_dim, y_dim), dt),
               "puzzle": np.empty(M, np.uint32), "loc": np.empty((M, 2), np.int32), "legal": np.empty(M, np.uint8)}
        o = _lib.SparcObserveOut(_ptr(out["visited"]), _ptr(out["agent"]), elem, x_dim, y_dim, 0, 0,
                                 _ptr(out["puzzle"]), _ptr(out["loc"]), _ptr(out["legal"]))
        self._check(self.lib.sparc_observe_records_host(self.ctx, ctypes.byref(info), _ptr(rec), M, ctypes.byref(o)))
        return out

    # ---------------------------------------------------------------- target reachability of records
    def _check_reach(self, M, x_dim, y_dim, plane, outputs):
        """The argument rules of sparc_reach_records_device that need no device (ValueError)."""
        if not 1 <= M < 2**31:
            raise ValueError("M must be in 1..2^31-1")
        if plane and (x_dim < self.table.x_max or y_dim < self.table.y_max or x_dim * y_dim > 256):
            raise ValueError(f"x_dim, y_dim must be at least {self.table.x_max}, {self.table.y_max} (the table's "
                             "largest lattice) with x_dim * y_dim <= 256")
        if all(x is None for x in outputs):
            raise ValueError("out: at least one output is needed")

    def reach_records_device(self, info, d_records, M, x_dim=None, y_dim=None, d_dist=None, d_action_dist=None,
                             d_live=None, d_size=None, d_plane=None):
        """sparc_reach_records_device: of M records the distance to the target [M], through each
        action [M][4], the actions that keep the target reachable [M] (bits 0-3), the size of the
        target's component [M] and the distance plane [M][x_dim][y_dim], all uint8 with REACH_NONE
        (255) for "no way", each may be None; reads the context's tables only (asynchronous)."""
        M = int(M)
        x_dim = self.table.x_max if x_dim is None else int(x_dim)
        y_dim = self.table.y_max if y_dim is None else int(y_dim)
        self._check_reach(M, x_dim, y_dim, d_plane is not None, (d_dist, d_action_dist, d_live, d_size, d_plane))
        out = _lib.SparcReachOut(d_dist, d_action_dist, d_live, d_size, d_plane, x_dim, y_dim)
        self._check(self.lib.sparc_reach_records_device(self.ctx, ctypes.byref(info), d_records, M, ctypes.byref(out)))

    def reach_records_host(self, info, records, plane=True, x_dim=None, y_dim=None):
        """Reach of host records [M, record_bytes]: a dict of host uint8 arrays ``dist`` [M],
        ``action_dist`` [M, 4], ``live`` [M], ``size`` [M] and, with ``plane``, ``plane``
        [M, x_dim, y_dim] (synchronous)."""
        rec = np.ascontiguousarray(records, np.uint8)
        if rec.ndim != 2 or rec.shape[1] != info.record_bytes or len(rec) < 1:
            raise ValueError(f"records must be [M, {info.record_bytes}] uint8 with M >= 1")
        M = len(rec)
        x_dim = self.table.x_max if x_dim is None else int(x_dim)
        y_dim = self.table.y_max if y_dim is None else int(y_dim)
        self._check_reach(M, x_dim, y_dim, bool(plane), (True,))
        out = {"dist": np.empty(M, np.uint8), "action_dist": np.empty((M, 4), np.uint8), "live": np.empty(M, np.uint8),
               "size": np.empty(M, np.uint8)}
        if plane:
            out["plane"] = np.empty((M, x_dim, y_dim), np.uint8)
        o = _lib.SparcReachOut(_ptr(out["dist"]), _ptr(out["action_dist"]), _ptr(out["live"]), _ptr(out["size"]),
                               _ptr(out["plane"]) if plane else None, x_dim, y_dim)
        self._check(self.lib.sparc_reach_records_host(self.ctx, ctypes.byref(info), _ptr(rec), M, ctypes.byref(o)))
        return out

    # ---------------------------------------------------------------- legal-move playouts of records
    def playout_device(self, info, d_records, M, K, L, seed=0, id0=0, flags=0, d_code=None, d_flags=None,
                       d_steps=None, d_first=None, d_end=None, d_return=None, d_trace=None, d_final=None,
                       d_stats=None):
        """sparc_playout_device: K playouts of at most L steps from each of M records, uniform over
        the legal actions; outputs [M * K] (trace [L][M * K], stats [M][4][4] accumulated), each
        may be None; reads the context's tables only (asynchronous)."""
        out = _lib.SparcPlayoutOut(d_code, d_flags, d_steps, d_first, d_end, d_return, d_trace, d_final, d_stats)
        self._check(self.lib.sparc_playout_device(self.ctx, ctypes.byref(info), d_records, int(M), int(K), int(L),
                                                  int(seed) & (2**64 - 1), int(id0) & (2**64 - 1), int(flags),
                                                  ctypes.byref(out)))

    def playout_host(self, info, records, K, L, seed=0, id0=0, flags=0, trace=False, final=False, stats=None):
        """Play out host records [M, record_bytes]: a dict of host arrays ``code`` int8, ``flags``
        uint8, ``steps`` uint16, ``first`` uint8, ``end`` uint8, ``ret`` int32 (each [M, K]),
        optionally ``trace`` [L, M, K] uint8 and ``final`` [M * K, record_bytes] uint8, and
        ``stats`` [M, 4, 4] int32: a fresh zeroed array, or the given one added to (synchronous)."""
        rec = np.ascontiguousarray(records, np.uint8)
        if rec.ndim != 2 or rec.shape[1] != info.record_bytes or len(rec) < 1:
            raise ValueError(f"records must be [M, {info.record_bytes}] uint8 with M >= 1")
        M, K, L = len(rec), int(K), int(L)
        if K < 1 or M * K >= 2**31 or not 1 <= L <= 65535 or K * L >= 2**31:
            raise ValueError("K >= 1, M * K < 2^31, 1 <= L <= 65535 and K * L < 2^31 are needed")
        if stats is None:
            stats = np.zeros((M, 4, 4), np.int32)
        elif not (isinstance(stats, np.ndarray) and stats.dtype == np.int32 and stats.shape == (M, 4, 4)
                  and stats.flags.c_contiguous):
            raise ValueError(f"stats must be a C-contiguous int32 array [{M}, 4, 4]")
        out = {"code": np.empty((M, K), np.int8), "flags": np.empty((M, K), np.uint8),
               "steps": np.empty((M, K), np.uint16), "first": np.empty((M, K), np.uint8),
               "end": np.empty((M, K), np.uint8), "ret": np.empty((M, K), np.int32), "stats": stats}
        if trace:
            out["trace"] = np.empty((L, M, K), np.uint8)
        if final:
            out["final"] = np.empty((M * K, rec.shape[1]), np.uint8)
        o = _lib.SparcPlayoutOut(_ptr(out["code"]), _ptr(out["flags"]), _ptr(out["steps"]), _ptr(out["first"]),
                                 _ptr(out["end"]), _ptr(out["ret"]), _ptr(out.get("trace")), _ptr(out.get("final")),
                                 _ptr(stats))
        self._check(self.lib.sparc_playout_host(self.ctx, ctypes.byref(info), _ptr(rec), M, K, L,
                                                int(seed) & (2**64 - 1), int(id0) & (2**64 - 1), int(flags),
                                                ctypes.byref(o)))
        return out

    # ---------------------------------------------------------------- replay of given action sequences
    @staticmethod
    def _check_replay(records, puzzle, M, L, actions, flags, outputs, per_step):
        """The argument rules of sparc_replay_device that need no device (ValueError)."""
        if (records is None) == (puzzle is None):
            raise ValueError("exactly one of records and puzzle must be given")
        if not 1 <= M < 2**31:
            raise ValueError("M must be in 1..2^31-1")
        if not 0 <= L <= 65535:
            raise ValueError("L must be in 0..65535")
        if flags & ~(_lib.REPLAY_STOP_DONE | _lib.REPLAY_STOP_ILLEGAL):
            raise ValueError("unknown bits in flags")
        if L == 0 and (actions is not None or any(x is not None for x in per_step)):
            raise ValueError("L = 0: actions, step_code, step_flags and states must be None")
        if L > 0 and actions is None:
            raise ValueError("actions are needed for L > 0")
        if all(x is None for x in outputs):
            raise ValueError("out: at least one output is needed")

    def replay_device(self, info, d_records, d_puzzle, M, L, d_actions, d_len=None, flags=0, d_code=None,
                      d_flags=None, d_steps=None, d_end=None, d_return=None, d_bad=None, d_step_code=None,
                      d_step_flags=None, d_final=None, d_states=None):
        """sparc_replay_device: M sequences of at most L given actions ([L][M] uint8, lengths d_len [M]
        uint32 or None), each from record j of d_records or from the reset state of puzzle
        d_puzzle[j] (exactly one of the two); outputs [M] (step_code, step_flags [L][M]; final [M]
        records, states [L][M] records), each may be None; reads the context's tables only
        (asynchronous)."""
        M, L, flags = int(M), int(L), int(flags)
        per_step = (d_step_code, d_step_flags, d_states)
        outs = (d_code, d_flags, d_steps, d_end, d_return, d_bad, d_final) + per_step
        self._check_replay(d_records, d_puzzle, M, L, d_actions, flags, outs, per_step)
        out = _lib.SparcReplayOut(d_code, d_flags, d_steps, d_end, d_return, d_bad, d_step_code, d_step_flags, d_final,
                                  d_states)
        self._check(self.lib.sparc_replay_device(self.ctx, ctypes.byref(info), d_records, d_puzzle, M, L, d_actions,
                                                 d_len, flags, ctypes.byref(out)))

    def replay_host(self, info, actions, records=None, puzzle=None, lengths=None, flags=0, per_step=False,
                    final=True, states=False):
        """Replay host action lists ``actions`` [L, M] uint8 from host records [M, record_bytes] or
        from the reset states of ``puzzle`` [M]: a dict of host arrays ``code`` int8, ``flags`` uint8,
        ``steps`` uint16, ``end`` uint8, ``ret`` int32, ``bad`` uint16 (each [M]), optionally
        ``step_code`` / ``step_flags`` [L, M], ``final`` [M, record_bytes] and ``states``
        [L * M, record_bytes] uint8 (synchronous)."""
        act = np.ascontiguousarray(actions, np.uint8)
        if act.ndim != 2:
            raise ValueError("actions must be [L, M] uint8")
        L, M = act.shape
        rec = None if records is None else np.ascontiguousarray(records, np.uint8)
        if rec is not None and (rec.ndim != 2 or rec.shape != (M, info.record_bytes)):
            raise ValueError(f"records must be [{M}, {info.record_bytes}] uint8")
        pz = None if puzzle is None else np.ascontiguousarray(puzzle, np.uint32)
        ln = None if lengths is None else np.ascontiguousarray(lengths, np.uint32)
        for a, what in ((pz, "puzzle"), (ln, "lengths")):
            if a is not None and a.shape != (M,):
                raise ValueError(f"{what} must have shape ({M},)")
        out = {"code": np.empty(M, np.int8), "flags": np.empty(M, np.uint8), "steps": np.empty(M, np.uint16),
               "end": np.empty(M, np.uint8), "ret": np.empty(M, np.int32), "bad": np.empty(M, np.uint16)}
        if per_step and L:
            out["step_code"], out["step_flags"] = np.empty((L, M), np.int8), np.empty((L, M), np.uint8)
        if final:
            out["final"] = np.empty((M, info.record_bytes), np.uint8)
        if states and L:
            out["states"] = np.empty((L * M, info.record_bytes), np.uint8)
        per = tuple(out.get(k) for k in ("step_code", "step_flags", "states"))
        self._check_replay(rec, pz, M, L, act if L else None, int(flags), tuple(out.values()), per)
        o = _lib.SparcReplayOut(*(_ptr(out.get(k)) for k in ("code", "flags", "steps", "end", "ret", "bad",
                                                              "step_code", "step_flags", "final", "states")))
        self._check(self.lib.sparc_replay_host(self.ctx, ctypes.byref(info), _ptr(rec), _ptr(pz), M, L,
                                               _ptr(act) if L else None, _ptr(ln), int(flags), ctypes.byref(o)))
        return out

    # ---------------------------------------------------------------- depth-first subtree search of records
    def dfs_device(self, info, d_records, M, budget, d_state, d_status, d_counts, d_cursor, d_first=None,
                   d_und_rec=None, d_und_root=None, d_und_count=None, und_cap=0, prune=None):
        """sparc_dfs_device: the forward-move subtree below each of M records, walked depth-first
        for at most ``budget`` nodes each, with the rule verdict of every target leaf; state [M]
        uint32 in/out, status [M] uint8, counts [M][8] uint64 accumulated, cursor [M] records,
        optionally first [M] records and the undecided leaves' buffer (all three pointers or none);
        reads the context's tables only (asynchronous).  With ``prune`` (the C value: 0, 1 =
        ``_lib.DFS_PRUNE_REACH`` or 3 = REACH | DEADLINE) sparc_dfs_pruned_device, which also holds a
        state word to the mode of its walk; None: sparc_dfs_device itself."""
        M, budget = int(M), int(budget)
        if not 1 <= budget < 2**32:
            raise ValueError("budget must be in 1..2^32-1")
        out = _lib.SparcDfsOut(d_status, d_counts, d_cursor, d_first, d_und_rec, d_und_root, d_und_count, int(und_cap))
        if prune is None:
            self._check(self.lib.sparc_dfs_device(self.ctx, ctypes.byref(info), d_records, M, budget, d_state,
                                                  ctypes.byref(out)))
        else:
            self._check(self.lib.sparc_dfs_pruned_device(self.ctx, ctypes.byref(info), d_records, M, budget,
                                                         int(prune), d_state, ctypes.byref(out)))

    def dfs_host(self, info, records, budget, state=None, counts=None, first=None, undecided=0, prune=None):
        """Walk host records [M, record_bytes] (synchronous): a dict of host arrays ``status`` [M]
        uint8, ``counts`` [M, 8] uint64, ``cursor`` and ``first`` [M, record_bytes] uint8, ``state``
        [M] uint32 and, with ``undecided`` > 0 (the buffer's entries), ``undecided``
        [n, record_bytes] uint8, ``undecided_root`` [n] uint32 and ``undecided_total``.  ``state``,
        ``counts`` and ``first`` of a previous call are continued in place (``records`` is then that
        call's ``cursor``); fresh zeroed arrays otherwise.  ``prune``: as ``dfs_device``
        (sparc_dfs_pruned_host unless None)."""
        rec = np.ascontiguousarray(records, np.uint8)
        if rec.ndim != 2 or rec.shape[1] != info.record_bytes or len(rec) < 1:
            raise ValueError(f"records must be [M, {info.record_bytes}] uint8 with M >= 1")
        M, budget, cap = len(rec), int(budget), int(undecided)
        if not 1 <= budget < 2**32:
            raise ValueError("budget must be in 1..2^32-1")
        if cap < 0:
            raise ValueError("undecided must not be negative")

        def arg(a, shape, dtype, what):
            if a is None:
                return np.zeros(shape, dtype)
            if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == shape and a.flags.c_contiguous):
                raise ValueError(f"{what} must be a C-contiguous {np.dtype(dtype).name} array {list(shape)}")
            return a

        state = arg(state, (M,), np.uint32, "state")
        counts = arg(counts, (M, _lib.DFS_COUNTERS), np.uint64, "counts")
        first = arg(first, rec.shape, np.uint8, "first")
        out = {"status": np.empty(M, np.uint8), "counts": counts, "cursor": np.empty_like(rec), "first": first,
               "state": state}
        und = np.empty((cap, rec.shape[1]), np.uint8) if cap else None
        root = np.empty(cap, np.uint32) if cap else None
        count = np.zeros(1, np.uint64) if cap else None
        o = _lib.SparcDfsOut(_ptr(out["status"]), _ptr(counts), _ptr(out["cursor"]), _ptr(first), _ptr(und),
                             _ptr(root), _ptr(count), cap)
        if prune is None:
            self._check(self.lib.sparc_dfs_host(self.ctx, ctypes.byref(info), _ptr(rec), M, budget, _ptr(state),
                                                ctypes.byref(o)))
        else:
            self._check(self.lib.sparc_dfs_pruned_host(self.ctx, ctypes.byref(info), _ptr(rec), M, budget,
                                                       int(prune), _ptr(state), ctypes.byref(o)))
        if cap:
            n = min(int(count[0]), cap)
            out.update(undecided=und[:n], undecided_root=root[:n], undecided_total=int(count[0]))
        return out

    # ---------------------------------------------------------------- UCT tree search of records
    @staticmethod
    def _check_mcts(M, sims, L, flags, T, cap):
        """The argument rules of sparc_mcts_device that need no device (ValueError naming the argument)."""
        if not 1 <= M < 2**31:
            raise ValueError("M must be in 1..2^31-1")
        if not 1 <= sims < 2**31:
            raise ValueError("sims must be in 1..2^31-1")
        if not 1 <= L <= 65535:
            raise ValueError("L (the horizon) must be in 1..65535")
        if flags & ~_lib.PLAYOUT_FORWARD:
            raise ValueError("unknown bits in flags")
        if T < 2:
            raise ValueError("T (the entries of ep and ec) must be at least 2")
        if not 1 <= cap <= _lib.MCTS_MAX_CAP:
            raise ValueError("cap must be in 1..2^24")
        if M * cap * 4 * _lib.MCTS_NODE_WORDS >= 2**63:
            raise ValueError("M * cap * 64 must fit in int64")

    def mcts_device(self, info, d_records, M, sims, L, d_ep, d_ec, T, cap, d_nodes, d_count, d_status, d_sims_done,
                    d_win_rec, d_win_steps, seed=0, id0=0, flags=0):
        """sparc_mcts_device: ``sims`` UCT simulations on the tree of each of M records, the trees in
        the arena d_nodes [M][cap] of 64-byte nodes with d_count [M] uint32 in use (in/out; 0: a fresh
        tree); ep, ec [T] float32 the exploration tables; status [M] uint8, sims_done [M] uint32,
        win_rec [M] records and win_steps [M] uint32 (both in/out), all needed; reads the context's
        tables only (asynchronous)."""
        M, sims, L, T, cap, flags = int(M), int(sims), int(L), int(T), int(cap), int(flags)
        self._check_mcts(M, sims, L, flags, T, cap)
        out = _lib.SparcMctsOut(d_status, d_sims_done, d_win_rec, d_win_steps)
        self._check(self.lib.sparc_mcts_device(self.ctx, ctypes.byref(info), d_records, M, sims, L,
                                               int(seed) & (2**64 - 1), int(id0) & (2**64 - 1), flags, d_ep, d_ec, T,
                                               cap, d_nodes, d_count, ctypes.byref(out)))

    def mcts_host(self, info, records, sims, L, ep, ec, cap, nodes=None, count=None, win=None, win_steps=None,
                  seed=0, id0=0, flags=0):
        """Search host records [M, record_bytes] (synchronous): a dict of host arrays ``status`` [M]
        uint8, ``sims`` [M] uint32 (this call's), ``nodes`` [M, cap, 16] uint32, ``count`` [M] uint32,
        ``win`` [M, record_bytes] uint8 and ``win_steps`` [M] uint32.  ``nodes``, ``count``, ``win``
        and ``win_steps`` of a previous call are continued in place; fresh ones (zeroed, win_steps
        0xFFFFFFFF) otherwise."""
        rec = np.ascontiguousarray(records, np.uint8)
        if rec.ndim != 2 or rec.shape[1] != info.record_bytes or len(rec) < 1:
            raise ValueError(f"records must be [M, {info.record_bytes}] uint8 with M >= 1")
        ep, ec = np.ascontiguousarray(ep, np.float32), np.ascontiguousarray(ec, np.float32)
        if ep.ndim != 1 or ep.shape != ec.shape:
            raise ValueError("ep and ec must be one-dimensional float32 arrays of the same length T")
        M, sims, L, T, cap, flags = len(rec), int(sims), int(L), len(ep), int(cap), int(flags)
        self._check_mcts(M, sims, L, flags, T, cap)

        def arg(a, shape, dtype, what, fill=0):
            if a is None:
                return np.full(shape, fill, dtype)
            if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == shape and a.flags.c_contiguous):
                raise ValueError(f"{what} must be a C-contiguous {np.dtype(dtype).name} array {list(shape)}")
            return a

        nodes = arg(nodes, (M, cap, _lib.MCTS_NODE_WORDS), np.uint32, "nodes")
        count = arg(count, (M,), np.uint32, "count")
        win = arg(win, rec.shape, np.uint8, "win")
        win_steps = arg(win_steps, (M,), np.uint32, "win_steps", 0xFFFFFFFF)
        out = {"status": np.empty(M, np.uint8), "sims": np.empty(M, np.uint32), "nodes": nodes, "count": count,
               "win": win, "win_steps": win_steps}
        o = _lib.SparcMctsOut(_ptr(out["status"]), _ptr(out["sims"]), _ptr(win), _ptr(win_steps))
        self._check(self.lib.sparc_mcts_host(self.ctx, ctypes.byref(info), _ptr(rec), M, sims, L,
                                             int(seed) & (2**64 - 1), int(id0) & (2**64 - 1), flags, _ptr(ep),
                                             _ptr(ec), T, cap, _ptr(nodes), _ptr(count), ctypes.byref(o)))
        return out


def visited_planes(bits, table: PuzzleTable, x_dim=None, y_dim=None):
    """Decode visited bitboards [words][N] into int32 planes [N][x_dim][y_dim] (host)."""
    W, n = bits.shape
    x_dim = table.x_max if x_dim is None else x_dim
    y_dim = table.y_max if y_dim is None else y_dim
    xs, ys = np.meshgrid(np.arange(x_dim), np.arange(y_dim), indexing="ij")
    b = xs * table.pitch + ys
    valid = (ys < table.pitch) & (b < 64 * W)
    b = np.where(valid, b, 0)
    words = bits[(b >> 6), :]                                   # [x, y, N]
    v = (words >> (b & 63).astype(np.uint64)[..., None]) & np.uint64(1)
    v = np.where(valid[..., None], v, 0).astype(np.int32)
    return np.ascontiguousarray(np.moveaxis(v, -1, 0))
