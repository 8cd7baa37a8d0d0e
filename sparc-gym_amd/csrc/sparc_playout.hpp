// sparc_playout.hpp — legal-move playouts of state records (device code): K independent random
// continuations of each of M records, played to the end of the episode or a horizon of L steps in
// one launch and without an env, with the root statistics a flat Monte-Carlo search or an MCTS
// needs.  The context supplies the tables, pitch and max_steps only.
//
//   One lane per playout: lane g = j * K + k plays playout k of record j, so the K playouts of a
//   record are neighbours and read the same record and puzzle rows.
//   The step is the project's own: as in k_expand the lane puts the parent's fields into ITS slot
//   of a 256-slot SoA in LDS, Env::load reads them, and from then on the Env stays in registers:
//   L times { mask of the legal actions (_get_legal_actions, SPaRC_Gym.py:1024-1051), a uniform
//   draw among its set bits (uint_rand_pick), Env::advance (step, 1111-1238) }.  A playout ends
//   with the step that terminates or truncates, so it never crosses an episode boundary and the
//   context's autoreset mode plays no part.  A wave leaves the loop when none of its lanes is
//   live; lanes whose playout ended idle until the longest playout of their wave ends.
//   Env::store then writes the slot once, the slot is read back, and the same LDS holds the
//   workgroup's 256 final records, stored as whole 16-B pieces of each wave's contiguous run
//   (k_snapshot, k_expand).  The per-step actions are stored step-major: 64 contiguous bytes
//   per wave and step.
//   Root statistics: per record and first action {playouts, +100 endings, -100 endings, steps},
//   packed into one 64-bit word per lane and action, summed over each record's lanes of the wave
//   with a segmented shuffle reduction, and added with one integer atomic per non-zero counter
//   by the segment's first lane: the result does not depend on the order.
//
// A parent record is checked with expand_record_ok before anything is indexed with it; a parent
// that fails gives end reason 0, zeroed outputs and raises kErrSnapshot.
#pragma once
#include "sparc_expand.hpp"

namespace sparc {

constexpr uint32_t kPlayoutForward = 1;   // SPARC_PLAYOUT_FORWARD: never draw the traceback pop

// end reasons (sparc_gym_amd.h SPARC_PLAYOUT_END_*)
constexpr uint32_t kEndInvalid = 0, kEndTerminated = 1, kEndTruncated = 2, kEndHorizon = 3, kEndDeadEnd = 4,
                   kEndPending = 5;

struct PlayoutOut {
    int8_t* __restrict__ code;       // [MK] the last step's reward code
    uint8_t* __restrict__ flags;     // [MK] the last step's flag byte
    uint16_t* __restrict__ steps;    // [MK] steps taken
    uint8_t* __restrict__ first;     // [MK] first action, 0xFF: none
    uint8_t* __restrict__ end;       // [MK] end reason
    int32_t* __restrict__ ret;       // [MK] sum of the reward codes
    uint8_t* __restrict__ trace;     // [L][MK] action of step t, 0xFF at and after the end
    uint4* __restrict__ final_rec;   // [MK] records
    int32_t* __restrict__ stats;     // [M][4][4] accumulated
};

// bit of the traceback pop in the legal mask: the direction back to path[-2], which legal_mask
// calls `back` (generic widths: the reverse of the last move; W = 1: rl, kept reversed); 0 where
// there is no pop
template <int W, bool TB>
__device__ __forceinline__ uint32_t pop_bit(const Env<W, TB>& e) {
    if constexpr (!TB) {
        return 0u;
    } else if constexpr (W == 1) {
        return e.len >= 2u ? 1u << e.rl : 0u;
    } else {
        return e.len >= 2u ? 1u << (e.last ^ 2u) : 0u;
    }
}

// Playout g = j * K + k of record j for g < MK (MK = M * K < 2^31), ids id0 + g.
template <int W, bool TB>
__global__ void __launch_bounds__(kSnapBlock) k_playout(Params p, const uint4* __restrict__ rec, uint32_t MK,
                                                        uint32_t K, uint32_t L, uint64_t seed, uint64_t id0,
                                                        uint32_t pflags, PlayoutOut o) {
    using R = SnapRec<W, TB>;
    constexpr int kD = TB ? 2 * W : 0;                       // direction-stack words of a slot
    static_assert((W + kD) * 8 + 16 <= R::kBytes, "an SoA slot fits in a record");
    __shared__ uint4 stage[kSnapBlock * R::kPieces];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t g = blockIdx.x * kSnapBlock + t;
    const bool in = g < MK;
    const uint32_t par = in ? g / K : 0xFFFFFFFFu;
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
    q.autoreset = 0;   // a playout stops at the done step: no step ever starts from a pending state
    const State& s = q.st;
    const PuzzleSrc<W> src{p.tab.info, p.tab.root, p.tab.open, p.tab.init, p.tab.row1};
    Env<W, TB> e;
    bool ok = false;
    if (in) {
        const uint4* pc = rec + (size_t)par * R::kPieces;
        uint32_t r[R::kWords];
#pragma unroll
        for (int k = 0; k < R::kPieces; ++k) {
            const uint4 v = pc[k];
            r[4 * k] = v.x;
            r[4 * k + 1] = v.y;
            r[4 * k + 2] = v.z;
            r[4 * k + 3] = v.w;
        }
        ok = expand_record_ok(p.tab, r[0], r[1], r[3]);
        if (ok) {
#pragma unroll
            for (int k = 0; k < W; ++k)
                s.vis[k * kSnapBlock + t] = r[R::kVis + 2 * k] | ((uint64_t)r[R::kVis + 2 * k + 1] << 32);
            if constexpr (TB) {
                const uint32_t len = (r[0] >> 16) & 0xFFu;
#pragma unroll
                for (int k = 0; k < kD; ++k) {
                    uint64_t d = r[R::kDirs + 2 * k] | ((uint64_t)r[R::kDirs + 2 * k + 1] << 32);
                    if constexpr (W == 1) d &= low_moves(len - 1u, k);   // canonical, as k_restore stores it
                    s.dirs[k * kSnapBlock + t] = d;
                }
            }
            s.pos[t] = r[0];
            s.aux[t] = r[1];
            s.step[t] = r[2];
            s.pid[t] = r[3];
            e.load(q, src, t);
        } else if (g - par * K == 0u) {
            atomicOr(p.err, (int)kErrSnapshot);
        }
    }
    uint32_t end = !ok ? kEndInvalid : (e.pending ? kEndPending : kEndHorizon);
    bool live = ok && !e.pending;
    const bool fwd_only = TB && (pflags & kPlayoutForward);
    const uint64_t id = id0 + g;
    int code = 0, ret = 0;
    uint32_t f = 0, steps = 0, first = 0xFFu;
    uint32_t ts = 0;
    for (; ts < L; ++ts) {
        if (__ballot(live) == 0ull) break;
        uint32_t a = 0xFFu;
        if (live) {
            uint32_t mask = e.legal;
            if (fwd_only) mask &= ~pop_bit<W, TB>(e);
            if (mask == 0u && e.legal != 0u) {
                end = kEndDeadEnd;
                live = false;
            } else {
                a = uint_rand_pick(seed, id, ts, mask);
                code = e.advance(q, src, a, f);
                ret += code;
                first = steps == 0u ? a : first;
                steps += 1u;
                if (f & 3u) {
                    end = (f & 1u) ? kEndTerminated : kEndTruncated;
                    live = false;
                }
            }
        }
        if (o.trace && in) o.trace[(size_t)ts * MK + g] = (uint8_t)a;
    }
    if (o.trace && in)
        for (; ts < L; ++ts) o.trace[(size_t)ts * MK + g] = 0xFFu;
    if (in) {
        if (o.code) o.code[g] = (int8_t)code;
        if (o.flags) o.flags[g] = (uint8_t)f;
        if (o.steps) o.steps[g] = (uint16_t)steps;
        if (o.first) o.first[g] = (uint8_t)first;
        if (o.end) o.end[g] = (uint8_t)end;
        if (o.ret) o.ret[g] = ret;
    }
    if (o.stats) {
        // segments of the wave: runs of lanes with the same record (lanes past MK: one empty run)
        const uint32_t prev = __shfl_up(par, 1);
        const uint64_t heads = __ballot(lane == 0u || prev != par);
        const uint64_t above = lane == 63u ? 0ull : heads & ~((2ull << lane) - 1ull);
        const uint32_t tail = above ? (uint32_t)__builtin_ctzll(above) - 1u : 63u;
        const bool head = (heads >> lane) & 1ull;
        // steps (22 bits: 64 * 65535) | playouts << 22 | +100 << 29 | -100 << 36 (7 bits each)
        const uint64_t mine = steps == 0u ? 0ull
                                          : (uint64_t)steps | (1ull << 22) | ((uint64_t)(code == 100) << 29) |
                                                ((uint64_t)(code == -100) << 36);
#pragma unroll
        for (uint32_t a = 0; a < 4; ++a) {
            uint64_t v = first == a ? mine : 0ull;
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint64_t u = __shfl_down(v, d);
                v += lane + d <= tail ? u : 0ull;
            }
            if (head && in && v != 0ull) {
                int32_t* row = o.stats + ((size_t)par * 4 + a) * 4;
                atomicAdd(row + 0, (int32_t)((v >> 22) & 0x7Fu));
                if ((v >> 29) & 0x7Fu) atomicAdd(row + 1, (int32_t)((v >> 29) & 0x7Fu));
                if ((v >> 36) & 0x7Fu) atomicAdd(row + 2, (int32_t)((v >> 36) & 0x7Fu));
                atomicAdd(row + 3, (int32_t)(v & 0x3FFFFFu));
            }
        }
    }
    if (!o.final_rec) return;   // the same for every thread of the grid
    uint32_t w[R::kWords];
#pragma unroll
    for (int k = 0; k < R::kWords; ++k) w[k] = 0;
    if (ok) {
        e.store(q, src, t);
        w[0] = s.pos[t];
        w[1] = s.aux[t];
        w[2] = s.step[t];
        w[3] = s.pid[t];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const uint64_t v = s.vis[k * kSnapBlock + t];
            w[R::kVis + 2 * k] = (uint32_t)v;
            w[R::kVis + 2 * k + 1] = (uint32_t)(v >> 32);
        }
        if constexpr (TB) {
#pragma unroll
            for (int k = 0; k < kD; ++k) {
                const uint64_t v = s.dirs[k * kSnapBlock + t];
                w[R::kDirs + 2 * k] = (uint32_t)v;
                w[R::kDirs + 2 * k + 1] = (uint32_t)(v >> 32);
            }
        }
    }
    __syncthreads();   // every slot has been read back: the LDS now takes the records
    uint4* wl = stage + wave * 64u * R::kPieces;
#pragma unroll
    for (int k = 0; k < R::kPieces; ++k)
        wl[lane * R::kPieces + k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    __syncthreads();
    // this wave's records are one contiguous run of the output: piece k*64 + lane per store
    const uint32_t g0 = blockIdx.x * kSnapBlock + wave * 64u;
    const uint32_t cnt = g0 < MK ? (MK - g0 < 64u ? MK - g0 : 64u) : 0u;
    uint4* run = o.final_rec + (size_t)g0 * R::kPieces;
#pragma unroll
    for (int k = 0; k < R::kPieces; ++k) {
        const uint32_t qi = (uint32_t)k * 64u + lane;
        if (qi < cnt * R::kPieces) run[qi] = wl[qi];
    }
}

}  // namespace sparc
