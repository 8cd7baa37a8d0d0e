// sparc_dfs.hpp — depth-first subtree search of state records with rule verdicts (device code): for
// each of M records the subtree of FORWARD moves below it is walked in pre-order under a node
// budget, every target leaf gets the puzzle's own verdict (the rule audit of sparc_rules.hpp), and
// only counters, a cursor and a few records leave the lane.  The memory cost does not depend on the
// tree: on a traceback context the record is the search stack, it carries the path's moves.
//
//   One lane per record, 256-lane workgroups.  As in k_playout the lane puts the record's fields
//   into ITS slot of a 256-slot SoA in LDS, Env::load reads them, and from then on the Env stays
//   in registers.  One trip of the loop is one of
//     enter  the lowest untried forward action (the legal actions, _get_legal_actions,
//            SPaRC_Gym.py:1024-1051, minus the traceback pop, pop_bit) through Env::advance: one
//            real step() (1111-1238) with its reward code and flags;
//     undo   back to the parent, which is NOT a step: the visited bit, the position, len, last / rl
//            and the trie state (off, or the parent node as the pop branch of advance finds it) are
//            put back, outcome = pending = 0 as in every live state, step - 1; it does not ask
//            whether the reference's pop is legal there (it is not from path length 2 onto a closed
//            start, nor out of a done leaf).  The next action tried is the undone move + 1.
//   so the walk is the lexicographic order of the action sequences and a node at depth d below the
//   root has step = root.step + d.  A node is a leaf when its step terminated (a TARGET leaf,
//   1192), truncated (max_steps or no legal move, 1134 / 1195) or when it is live without a
//   forward move (a dead end).  The walk never undoes above the root's path length.
//   A target leaf is audited in place, on the board and agent the lane holds: audit<W, NoMemo>,
//   or audit_r's table-only form on a one-word pool whose every puzzle has a region-code table
//   (TABLE_ONLY: no exact-fit search compiled in).  puzzle_rules is loaded once per lane.  The
//   audit sits behind a wave-level ballot: a wave with no lane on a target skips it.  The
//   RulesTab has no exact-fit queue (fq.count null): a leaf whose search passed the node cap, or
//   whose puzzle is host-only without an answer in HostFits, is UNDECIDED: counted, and its record
//   appended to the caller's buffer (one 64-bit atomicAdd for the slot).
//   A lane enters at most `budget` nodes per call and finishes the accounting of the last one.
//   It then puts the cursor (that node) into its slot and only looks ahead: undos, no entry.  If
//   they reach the root with nothing left the walk is COMPLETE in this call; at the first
//   untried forward move the lane stops with the stored cursor.  So k calls of budget B do exactly
//   the first k * B nodes of the pre-order walk, and every loop here is bounded by the budget
//   (2 * budget + the longest path trips), the audit's own exact-fit node cap apart.
//   A wave leaves the loop when none of its lanes is live.
//
// Records written (cursor, first satisfied, undecided) go through Env::store into the lane's slot
// and are read back from it, so they are byte for byte what restore of the root, step with the
// forward actions and snapshot give (W = 1: the canonical stored form).  At W > 1 the stack
// fields at and above the top are written as zero (the walk has passed through them), which is
// what that sequence gives for every root whose own fields above the top are zero.  The cursors
// are stored as whole 16-B pieces of each wave's contiguous run (k_snapshot, k_playout).
//
// A record is checked with expand_record_ok, and its puzzle against the rule table's count (as
// k_rules_rec), before anything is indexed with it; a continued one also needs root length <= len.
#pragma once
#include "sparc_playout.hpp"
#include "sparc_rules.hpp"

namespace sparc {

// status (sparc_gym_amd.h SPARC_DFS_*)
constexpr uint32_t kDfsInvalid = 0, kDfsComplete = 1, kDfsBudget = 2, kDfsPending = 3, kDfsOverflow = 4;
enum : uint32_t { kDfsNodes = 0, kDfsTargets, kDfsSatisfied, kDfsListed, kDfsBoth, kDfsDeadEnds, kDfsTruncated,
                  kDfsUndecided, kDfsCounters };
// the state word: root path length | next action << 8 | flags
constexpr uint32_t kDfsNextShift = 8, kDfsDone = 1u << 28, kDfsFound = 1u << 29, kDfsLeaf = 1u << 30,
                   kDfsStarted = 1u << 31;
constexpr uint32_t kDfsModeShift = 12;   // bits 12-13: the walk's prune mode (0: every forward move)
constexpr uint32_t kDfsPruneReach = 1, kDfsPruneDeadline = 2;   // SPARC_DFS_PRUNE_*
constexpr uint32_t kRuleAllBit = 1u << 8, kRuleExhaustedBit = 1u << 9;   // SPARC_RULE_ALL, _SEARCH_EXHAUSTED

struct DfsOut {
    uint8_t* __restrict__ status;               // [M]
    unsigned long long* __restrict__ counts;    // [M][kDfsCounters] accumulated
    uint4* cursor;                              // [M] records; may alias the input
    uint4* __restrict__ first_sat;              // [M] records or null
    uint4* __restrict__ und_rec;                // [und_cap] records or null
    uint32_t* __restrict__ und_root;            // [und_cap]
    unsigned long long* __restrict__ und_count;
    uint64_t und_cap;
};

// the prune mode of a children policy (0 where it has none)
template <class Moves>
__device__ __forceinline__ uint32_t dfs_mode(const Moves& mv) {
    if constexpr (Moves::kPrune) return mv.mode;
    else return 0u;
}

// the forward moves of the state: its legal actions without the traceback pop
template <int W>
__device__ __forceinline__ uint32_t dfs_children(const Env<W, true>& e) {
    return e.legal & ~pop_bit<W, true>(e) & 15u;
}

// the last move of the path (len >= 2) as an action
template <int W>
__device__ __forceinline__ uint32_t dfs_last_move(const Env<W, true>& e) {
    if constexpr (W == 1) return e.rl ^ 2u;
    else return e.last;
}

// back to the parent of a node with len >= 2 (see the head of this file)
template <int W>
__device__ __forceinline__ void dfs_undo(Env<W, true>& e, const Params& p) {
    const uint32_t a = e.last;
    bb_clear<W>(e.vis, e.x * p.pitch + e.y);
    e.x = (uint32_t)((int)e.x - dir_dx(a));
    e.y = (uint32_t)((int)e.y - dir_dy(a));
    e.len -= 1;
    e.last = e.len >= 2u ? e.dir_at(e.len - 2u) : 0u;
    if (e.off > 0) {
        e.off -= 1;
    } else if (e.pflags & 2u) {
        e.node_term = rec_parent_term(e.rec);
        e.node = rec_parent(e.rec);
        e.load_rec(p);
    }
    e.outcome = 0;
    e.pending = 0;
    e.step -= 1;
    e.legal = e.legal_mask(p.pitch);
}
__device__ __forceinline__ void dfs_undo(Env<1, true>& e, const Params& p) {
    const uint32_t P = p.pitch;
    const uint32_t b = e.rl;                                           // the direction back to the parent
    e.fr |= 1ull << ((e.e + P) & 63u);                                 // the point left is free again
    e.e = e.e + __builtin_amdgcn_ubfe(p.nbr_pos, b << 3, 8u) - P;
    e.len -= 1;
    if (e.off > 0) {
        e.off -= 1;
    } else {                                                           // the parent: field[b] of the record
        e.nn = (uint32_t)((((uint64_t)e.rec.y << 32) | e.rec.x) >> ((b << 4) & 63u)) & 0xFFFFu;
    }
    e.load_rec(p);
    e.rl = e.len >= 2u ? e.stk.read(e.len - 2u) : 0u;
    e.pnr = e.stk.read(__builtin_elementwise_sub_sat(e.len, 3u));
    e.outcome = 0;
    e.pending = 0;
    e.step -= 1;
    e.legal = e.legal_mask(P);
    e.s_a = e.s_fwd = e.s_pop = e.s_mv = e.s_rs = e.s_done = 0;
}

// mask of the fields of `moves` moves that live in stack word `word` (32 moves per word)
__device__ __forceinline__ uint64_t dfs_low_moves(uint32_t moves, uint32_t word) {
    const uint32_t lo = word * 32u;
    const uint32_t m = moves > lo ? (moves - lo < 32u ? moves - lo : 32u) : 0u;
    return m >= 32u ? ~0ull : ((1ull << (2u * m)) - 1ull);
}

// the record held by slot t of the workgroup's SoA
template <int W>
__device__ __forceinline__ void dfs_slot_record(const State& s, uint32_t t, uint32_t (&w)[SnapRec<W, true>::kWords]) {
    using R = SnapRec<W, true>;
#pragma unroll
    for (int k = 0; k < R::kWords; ++k) w[k] = 0;
    w[0] = s.pos[t];
    w[1] = s.aux[t];
    w[2] = s.step[t];
    w[3] = s.pid[t];
    const uint32_t moves = ((w[0] >> 16) & 0xFFu) - 1u;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const uint64_t v = s.vis[k * kSnapBlock + t];
        w[R::kVis + 2 * k] = (uint32_t)v;
        w[R::kVis + 2 * k + 1] = (uint32_t)(v >> 32);
    }
#pragma unroll
    for (int k = 0; k < 2 * W; ++k) {
        const uint64_t v = s.dirs[k * kSnapBlock + t] & dfs_low_moves(moves, k);
        w[R::kDirs + 2 * k] = (uint32_t)v;
        w[R::kDirs + 2 * k + 1] = (uint32_t)(v >> 32);
    }
}

// Which children a node of the walk has: every forward move (the search of sparc_dfs_device; with this
// policy k_dfs compiles to what it was without one).  The pruned walk's policy (DfsLiveMoves,
// sparc_dfs_prune.hpp) has kPrune set, a `mode` and a wave-collective moves<W>(e, p, ask); the lines
// under `Moves::kPrune` below are that walk's and are described there.
struct DfsAllMoves {
    static constexpr bool kPrune = false;
};

// Record j < M (M < 2^31): see the head of this file and sparc_dfs_device (sparc_gym_amd.h).  `mv`: the
// children policy, DfsAllMoves (an empty argument) for the search of sparc_dfs_device.
template <int W, bool TABLE_ONLY, class Moves = DfsAllMoves>
__global__ void __launch_bounds__(kSnapBlock) k_dfs(Params p, RulesTab rt, const uint4* rec, uint32_t M,
                                                    uint32_t budget, uint32_t* __restrict__ state, DfsOut o,
                                                    Moves mv) {
    static_assert(!TABLE_ONLY || W == 1, "the table-only audit is the one-word one");
    using R = SnapRec<W, true>;
    constexpr int kD = 2 * W;
    static_assert((W + kD) * 8 + 16 <= R::kBytes, "an SoA slot fits in a record");
    __shared__ uint4 stage[kSnapBlock * R::kPieces];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t j = blockIdx.x * kSnapBlock + t;
    const bool in = j < M;
    // the workgroup's SoA in LDS, seen through Params as Env::load / store see the global one
    Params q = p;
    uint64_t* const l64 = reinterpret_cast<uint64_t*>(stage);
    uint32_t* const l32 = reinterpret_cast<uint32_t*>(l64 + (W + kD) * kSnapBlock);
    q.st.vis = l64;
    q.st.dirs = l64 + W * kSnapBlock;
    q.st.pos = l32;
    q.st.aux = l32 + kSnapBlock;
    q.st.step = l32 + 2 * kSnapBlock;
    q.st.pid = l32 + 3 * kSnapBlock;
    q.n = kSnapBlock;
    q.autoreset = 0;   // a done leaf is left by the undo, never by a step
    const State& s = q.st;
    const PuzzleSrc<W> src{p.tab.info, p.tab.root, p.tab.open, p.tab.init, p.tab.row1};
    Env<W, true> e;
    PuzzleRules<W> pr;
    const uint32_t st0 = in ? state[j] : kDfsDone;
    const bool was_done = (st0 & kDfsDone) != 0u;
    bool ok = false;
    if (in && !was_done) {
        const uint4* pc = rec + (size_t)j * R::kPieces;
        uint32_t r[R::kWords];
#pragma unroll
        for (int k = 0; k < R::kPieces; ++k) {
            const uint4 v = pc[k];
            r[4 * k] = v.x;
            r[4 * k + 1] = v.y;
            r[4 * k + 2] = v.z;
            r[4 * k + 3] = v.w;
        }
        const uint32_t len = (r[0] >> 16) & 0xFFu;
        if (!expand_record_ok(p.tab, r[0], r[1], r[3])) {
            atomicOr(p.err, (int)kErrSnapshot);
        } else if (r[3] >= rt.num_puzzles) {
            atomicOr(p.err, (int)kErrRuleTable);
        } else if (st0 != 0u && ((st0 & 0xFFu) < 1u || (st0 & 0xFFu) > len)) {
            atomicOr(p.err, (int)kErrSnapshot);   // a cursor above its own root
        } else if (Moves::kPrune && st0 != 0u && ((st0 >> kDfsModeShift) & 3u) != dfs_mode(mv)) {
            atomicOr(p.err, (int)kErrSnapshot);   // a cursor of a walk of another mode
        } else {
            ok = true;
#pragma unroll
            for (int k = 0; k < W; ++k)
                s.vis[k * kSnapBlock + t] = r[R::kVis + 2 * k] | ((uint64_t)r[R::kVis + 2 * k + 1] << 32);
#pragma unroll
            for (int k = 0; k < kD; ++k) {
                uint64_t d = r[R::kDirs + 2 * k] | ((uint64_t)r[R::kDirs + 2 * k + 1] << 32);
                if constexpr (W == 1) d &= low_moves(len - 1u, k);   // canonical, as k_restore stores it
                s.dirs[k * kSnapBlock + t] = d;
            }
            s.pos[t] = r[0];
            s.aux[t] = r[1];
            s.step[t] = r[2];
            s.pid[t] = r[3];
            e.load(q, src, t);
            pr = puzzle_rules<W>(p, rt, r[3]);
        }
    }
    // what the audit of a one-word state needs besides the free board
    uint64_t open0 = 0;
    uint32_t sbit = 0;
    if constexpr (W == 1) {
        if (ok) {
            open0 = p.tab.open[e.pid];
            sbit = src.get_row1(e.pid).x & 0xFFu;
        }
    }
    uint32_t status = was_done ? kDfsComplete : kDfsInvalid;
    uint32_t root_len = 0, next = 0;
    bool live = false, found = false, owe = false;
    // the pruned walk: the moves of the node the lane stands on (valid unless `need`), and whether
    // that node still owes its dead-end test (the root, or a node entered on the trip before)
    uint32_t moves = 0;
    bool need = true, fresh = false;
    uint32_t cnt[kDfsCounters];
#pragma unroll
    for (int k = 0; k < (int)kDfsCounters; ++k) cnt[k] = 0;
    if (ok) {
        if (st0 == 0u) {                                      // a fresh start: the record is the root
            root_len = e.len;
            if (e.pending) {
                status = kDfsPending;
            } else if constexpr (Moves::kPrune) {
                live = true;                                  // its moves are asked for in the loop
                fresh = true;
            } else if (dfs_children<W>(e) == 0u) {
                cnt[kDfsDeadEnds] = 1;
                status = kDfsComplete;
            } else {
                live = true;
            }
        } else {
            root_len = st0 & 0xFFu;
            next = (st0 >> kDfsNextShift) & 7u;
            found = (st0 & kDfsFound) != 0u;
            owe = (st0 & kDfsLeaf) != 0u;
            live = true;
        }
    }
    uint32_t entered = 0;
    bool ahead = false;   // the budget is spent and the cursor stored: undos only, looking for the end
    const uint64_t trips = 2ull * budget + 600ull;
    for (uint64_t it = 0; it < trips; ++it) {
        if (__ballot(live) == 0ull) break;
        if constexpr (Moves::kPrune) {
            // Every lane of the wave takes part (the flood leaves on a ballot); a lane with nothing
            // to ask passes an empty board.  The loop itself is left on a ballot only.
            const bool ask = live && !owe && need && !e.pending;
            if (__ballot(ask) != 0ull) {
                const uint32_t m = mv.template moves<W>(e, p, ask);
                if (ask) {
                    moves = m;
                    need = false;
                    if (fresh && m == 0u) cnt[kDfsDeadEnds] += 1u;
                    fresh = false;
                }
            }
        }
        bool tgt = false;
        if (live) {
            if (owe) {
                tgt = true;                                   // the leaf an overflow left unaccounted
            } else {
                uint32_t cand;
                if constexpr (Moves::kPrune) cand = e.pending ? 0u : (moves >> next) << next;
                else cand = e.pending ? 0u : (dfs_children<W>(e) >> next) << next;
                if (cand != 0u) {
                    if (ahead) {
                        live = false;                         // more to walk: the stored cursor stands
                        status = kDfsBudget;
                    } else {
                        uint32_t f = 0;
                        e.advance(q, src, (uint32_t)__builtin_ctz(cand), f);
                        next = 0;
                        entered += 1u;
                        cnt[kDfsNodes] += 1u;
                        if (f & 1u) tgt = true;
                        else if (f & 2u) cnt[kDfsTruncated] += 1u;
                        else if constexpr (Moves::kPrune) fresh = true;   // its dead-end test: the next trip
                        else if (dfs_children<W>(e) == 0u) cnt[kDfsDeadEnds] += 1u;
                        need = true;
                    }
                } else if (e.len <= root_len) {
                    live = false;
                    status = kDfsComplete;
                } else {
                    const uint32_t a = dfs_last_move<W>(e);
                    dfs_undo(e, q);
                    next = a + 1u;
                    need = true;                              // the parent's moves: one flood per trip
                }
            }
        }
        if (__ballot(tgt) != 0ull) {
            if (tgt) {
                uint32_t bits;
                BB<W> vis;
                if constexpr (W == 1) {
                    vis.w[0] = ((~e.fr >> p.pitch) & open0) | (1ull << sbit);   // as Env::store writes it
                    if constexpr (TABLE_ONLY) {
                        bits = audit_r<1, NoMemo, true>(p, rt, pr, vis, true, nullptr, nullptr).bits;
                    } else {
                        const uint32_t xy = e.agent_xy(p);
                        bits = audit<1, NoMemo>(p, rt, pr, vis, xy & 0xFFu, xy >> 8, nullptr, nullptr, 0).bits;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < W; ++k) vis.w[k] = e.vis[k];
                    bits = audit<W, NoMemo>(p, rt, pr, vis, e.x, e.y, nullptr, nullptr, 0).bits;
                }
                const bool und = (bits & kRuleExhaustedBit) != 0u;
                const bool listed = e.outcome == 1u;          // the step's code was +100
                bool fits = true;
                if (und && o.und_rec) {
                    const unsigned long long k = atomicAdd(o.und_count, 1ull);
                    if (k < o.und_cap) {
                        e.store(q, src, t);
                        uint32_t w[R::kWords];
                        dfs_slot_record<W>(s, t, w);
                        uint4* dst = o.und_rec + (size_t)k * R::kPieces;
#pragma unroll
                        for (int i = 0; i < R::kPieces; ++i)
                            dst[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
                        o.und_root[k] = j;
                    } else {
                        fits = false;                         // the cursor is this leaf, its accounting owed
                        owe = true;
                        live = false;
                        status = kDfsOverflow;
                    }
                }
                if (fits) {
                    owe = false;
                    cnt[kDfsTargets] += 1u;
                    cnt[kDfsListed] += (uint32_t)listed;
                    if (und) {
                        cnt[kDfsUndecided] += 1u;
                    } else if (bits & kRuleAllBit) {
                        cnt[kDfsSatisfied] += 1u;
                        cnt[kDfsBoth] += (uint32_t)listed;
                        if (!found && o.first_sat) {
                            e.store(q, src, t);
                            uint32_t w[R::kWords];
                            dfs_slot_record<W>(s, t, w);
                            uint4* dst = o.first_sat + (size_t)j * R::kPieces;
#pragma unroll
                            for (int i = 0; i < R::kPieces; ++i)
                                dst[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
                        }
                        found = true;
                    }
                }
            }
        }
        if (live && !ahead && entered >= budget) {
            e.store(q, src, t);                               // the cursor: node `budget` of this call
            ahead = true;
        }
    }
    if (live) status = kDfsBudget;                            // (the trip bound: not reached by a walk)
    // the slot holds the cursor already where the look-ahead ended at an untried move
    if (ok && !(ahead && status == kDfsBudget)) e.store(q, src, t);
    uint32_t w[R::kWords];
#pragma unroll
    for (int k = 0; k < R::kWords; ++k) w[k] = 0;
    if (ok) {
        dfs_slot_record<W>(s, t, w);
    } else if (in && was_done) {                              // left alone: the cursor is the record
        const uint4* pc = rec + (size_t)j * R::kPieces;
#pragma unroll
        for (int k = 0; k < R::kPieces; ++k) {
            const uint4 v = pc[k];
            w[4 * k] = v.x;
            w[4 * k + 1] = v.y;
            w[4 * k + 2] = v.z;
            w[4 * k + 3] = v.w;
        }
    }
    if (in) {
        o.status[j] = (uint8_t)status;
        if (!was_done) {
            uint32_t stw = kDfsStarted | kDfsDone;            // an invalid record is never walked again
            if (ok) {
                const bool done = status == kDfsComplete || status == kDfsPending;
                const uint32_t nx = status == kDfsBudget && !ahead ? next : 0u;   // a stored cursor is a fresh node
                stw = kDfsStarted | root_len | (nx << kDfsNextShift) | (done ? kDfsDone : 0u) |
                      (found ? kDfsFound : 0u) | (owe ? kDfsLeaf : 0u);
                if constexpr (Moves::kPrune) stw |= dfs_mode(mv) << kDfsModeShift;
            }
            state[j] = stw;
#pragma unroll
            for (int k = 0; k < (int)kDfsCounters; ++k)
                if (cnt[k]) o.counts[(size_t)j * kDfsCounters + k] += cnt[k];
        }
    }
    __syncthreads();   // every slot has been read back: the LDS now takes the records
    uint4* wl = stage + wave * 64u * R::kPieces;
#pragma unroll
    for (int k = 0; k < R::kPieces; ++k)
        wl[lane * R::kPieces + k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    __syncthreads();
    // this wave's cursors are one contiguous run of the output: piece k*64 + lane per store
    const uint32_t g0 = blockIdx.x * kSnapBlock + wave * 64u;
    const uint32_t n = g0 < M ? (M - g0 < 64u ? M - g0 : 64u) : 0u;
    uint4* run = o.cursor + (size_t)g0 * R::kPieces;
#pragma unroll
    for (int k = 0; k < R::kPieces; ++k) {
        const uint32_t qi = (uint32_t)k * 64u + lane;
        if (qi < n * R::kPieces) run[qi] = wl[qi];
    }
}

}  // namespace sparc
