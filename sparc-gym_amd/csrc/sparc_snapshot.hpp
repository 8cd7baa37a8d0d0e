// sparc_snapshot.hpp — snapshot / restore / fork of the batched env state (device code).
//
// The reference has no counterpart: its user copies the SPaRC_Gym object (the per-episode fields
// of _load_puzzle, SPaRC_Gym.py:141-187) to try a continuation and come back.  Here the state
// between launches is the SoA of sparc_env.hpp (State), and a snapshot is one fixed-size RECORD
// per env, array-of-structures, in caller-owned memory:
//
//   u32 word  0       pos   x | y<<8 | len<<16 | off<<24
//             1       aux   node | outcome<<16 | pending<<18 | node_term<<19
//             2       step
//             3       pid
//             4 ..    vis   W u64 words
//             then    dirs  2W u64 words (traceback only)
//             padding to a multiple of 16 B (zero)
//
// The four scalars lead, so that the restore validates a record from its first 16-B piece.
//   k_snapshot  SoA -> records.  A lane that wrote its own record would make stride-record_bytes
//               stores; instead each wave stages its 64 records in LDS and stores them as whole
//               16-B pieces of one contiguous run (piece k*64 + lane), as the I/O tiles of
//               k_rollout do.  With an env list the SoA reads are gathers, without it coalesced.
//   k_restore   records -> SoA.  A gather of one record per env, read as 16-B pieces (one or two
//               cache lines per env); the record is validated before anything is indexed with
//               it, the SoA stores are coalesced, and the legal mask of the restored state is
//               computed from the restored board as Env::load does.
// A fork is k_snapshot of every env into a context-owned scratch (coalesced), then k_restore of
// record src[i] into env i: every read of the state precedes every write, and the gather runs on
// the records (one or two lines per env), not on the seven SoA arrays.
#pragma once
#include "sparc_env.hpp"

namespace sparc {

constexpr uint32_t kErrSnapshot = 32;   // Params::err bit (sparc_sync): bad index or record in a restore / fork
constexpr int kSnapBlock = 256;

template <int W, bool TB>
struct SnapRec {
    static constexpr int kVis = 4;                          // first u32 word of the visited board
    static constexpr int kDirs = 4 + 2 * W;                 // ... of the direction stack
    static constexpr int kFields = 4 + 2 * W + (TB ? 4 * W : 0);
    static constexpr int kWords = (kFields + 3) & ~3;       // u32 words, padded to 16 B
    static constexpr int kPieces = kWords / 4;              // 16-B pieces
    static constexpr int kBytes = kWords * 4;
};

__host__ __device__ constexpr int snap_record_bytes(int W, bool tb) {
    return (((4 + 2 * W + (tb ? 4 * W : 0)) + 3) & ~3) * 4;
}

// The legal actions (_get_legal_actions, SPaRC_Gym.py:1024-1051; a 4-bit mask in action order) of
// the state of a VALIDATED record, from its board as Env::load finds them: pos and pid are the
// record's words, vis its visited board, `last` the path's last move (move len - 2 of the
// direction stack; only read under traceback with len >= 2, where the one legal revisit is its
// reverse).  k_restore's flags and k_observe_rec's legal byte.
template <int W, bool TB>
__device__ __forceinline__ uint32_t record_legal(const Params& p, uint32_t pos, uint32_t pid, const uint64_t (&vis)[W],
                                                 uint32_t last) {
    const uint32_t x = pos & 0xFFu, y = (pos >> 8) & 0xFFu, len = (pos >> 16) & 0xFFu;
    const PuzzleSrc<W> ps{p.tab.info, p.tab.root, p.tab.open, p.tab.init, p.tab.row1};
    Env<W, TB> e;
    if constexpr (W == 1) {
        const uint32_t P = p.pitch;
        e.e = x * P + y;
        e.len = len;
        e.load_puzzle(ps, pid);
        e.fr = (p.tab.open[pid] & ~vis[0]) << P;
        e.rl = (TB && len >= 2u) ? (last ^ 2u) : 0u;   // the stack in registers holds reversed moves
        return e.legal_mask(P);
    } else {
#pragma unroll
        for (int k = 0; k < W; ++k) e.vis[k] = vis[k];
        e.x = x;
        e.y = y;
        e.len = len;
        uint32_t sx, sy;
        e.load_puzzle(ps, pid, sx, sy);
        e.last = (TB && len >= 2u) ? last : 0u;
        return e.legal_mask(p.pitch);
    }
}

// Record j <- env env[j] (env NULL: env j) for j < M.  A record whose env index is not below N
// (error bit raised) is written as zeros: len 0, which no restore accepts.
template <int W, bool TB>
__global__ void __launch_bounds__(kSnapBlock) k_snapshot(Params p, const uint32_t* __restrict__ env, uint32_t M,
                                                         uint4* __restrict__ out) {
    using R = SnapRec<W, TB>;
    __shared__ uint4 stage[kSnapBlock * R::kPieces];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t j = blockIdx.x * kSnapBlock + threadIdx.x;
    uint4* wl = stage + wave * 64u * R::kPieces;
    uint32_t w[R::kWords];
#pragma unroll
    for (int k = 0; k < R::kWords; ++k) w[k] = 0;
    if (j < M) {
        const uint32_t i = env ? env[j] : j;
        if (i >= p.n) {
            atomicOr(p.err, (int)kErrSnapshot);
        } else {
            const State& s = p.st;
            w[0] = s.pos[i];
            w[1] = s.aux[i];
            w[2] = s.step[i];
            w[3] = s.pid[i];
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const uint64_t v = s.vis[(size_t)k * p.n + i];
                w[R::kVis + 2 * k] = (uint32_t)v;
                w[R::kVis + 2 * k + 1] = (uint32_t)(v >> 32);
            }
            if constexpr (TB) {
#pragma unroll
                for (int k = 0; k < 2 * W; ++k) {
                    const uint64_t v = s.dirs[(size_t)k * p.n + i];
                    w[R::kDirs + 2 * k] = (uint32_t)v;
                    w[R::kDirs + 2 * k + 1] = (uint32_t)(v >> 32);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < R::kPieces; ++k)
        wl[lane * R::kPieces + k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    __syncthreads();
    // this wave's records are one contiguous run of the output: piece k*64 + lane per store
    const uint32_t j0 = blockIdx.x * kSnapBlock + wave * 64u;
    const uint32_t cnt = j0 < M ? (M - j0 < 64u ? M - j0 : 64u) : 0u;
    uint4* run = out + (size_t)j0 * R::kPieces;
#pragma unroll
    for (int k = 0; k < R::kPieces; ++k) {
        const uint32_t q = (uint32_t)k * 64u + lane;
        if (q < cnt * R::kPieces) run[q] = wl[q];
    }
}

// Env i <- record src[i] (src NULL: record i) for i < N with mask[i] != 0 (mask NULL: all).
// Checked before anything is dereferenced with it: the record index (< M) and the record's
// fields that later kernels index tables and stacks with: pid < P, the trie node below the
// puzzle's node count (0 on a puzzle without a root), x < x_size, y < y_size, 1 <= len <= the
// lattice's points.  An env that fails keeps its state, and kErrSnapshot is raised.
template <int W, bool TB>
__global__ void __launch_bounds__(kSnapBlock) k_restore(Params p, const uint4* __restrict__ rec, uint32_t M,
                                                        const uint32_t* __restrict__ src,
                                                        const uint8_t* __restrict__ mask, uint8_t* __restrict__ flg) {
    using R = SnapRec<W, TB>;
    const uint32_t i = blockIdx.x * kSnapBlock + threadIdx.x;
    if (i >= p.n) return;
    if (mask && !mask[i]) return;
    const uint32_t r = src ? src[i] : i;
    if (r >= M) {
        atomicOr(p.err, (int)kErrSnapshot);
        return;
    }
    const uint4* pc = rec + (size_t)r * R::kPieces;
    uint32_t w[R::kWords];
#pragma unroll
    for (int k = 0; k < R::kPieces; ++k) {
        const uint4 v = pc[k];
        w[4 * k] = v.x;
        w[4 * k + 1] = v.y;
        w[4 * k + 2] = v.z;
        w[4 * k + 3] = v.w;
    }
    const uint32_t pos = w[0], aux = w[1], pid = w[3];
    const uint32_t x = pos & 0xFFu, y = (pos >> 8) & 0xFFu, len = (pos >> 16) & 0xFFu;
    bool ok = pid < p.tab.num_puzzles;
    if (ok) {
        const uint4 inf = p.tab.info[pid];
        const uint32_t X = inf.x & 0xFFu, Y = (inf.x >> 8) & 0xFFu;
        const uint32_t nodes = ((inf.y >> 16) & 2u) ? (inf.w & 0xFFFFu) : 1u;
        ok = x < X && y < Y && len >= 1u && len <= X * Y && (aux & 0xFFFFu) < nodes;
    }
    if (!ok) {
        atomicOr(p.err, (int)kErrSnapshot);
        return;
    }
    uint64_t vis[W], dirs[TB ? 2 * W : 1];
#pragma unroll
    for (int k = 0; k < W; ++k) vis[k] = w[R::kVis + 2 * k] | ((uint64_t)w[R::kVis + 2 * k + 1] << 32);
    if constexpr (TB) {
#pragma unroll
        for (int k = 0; k < 2 * W; ++k) dirs[k] = w[R::kDirs + 2 * k] | ((uint64_t)w[R::kDirs + 2 * k + 1] << 32);
        // W = 1 keeps the stack canonical in HBM: only the path's len - 1 moves set
        // (RegStack::store); the generic step path stores its words as they are, so there the
        // record's words are too
        if constexpr (W == 1) {
            dirs[0] &= low_moves(len - 1u, 0);
            dirs[1] &= low_moves(len - 1u, 1);
        }
    } else {
        dirs[0] = 0;
    }
    const State& s = p.st;
#pragma unroll
    for (int k = 0; k < W; ++k) s.vis[(size_t)k * p.n + i] = vis[k];
    if constexpr (TB) {
#pragma unroll
        for (int k = 0; k < 2 * W; ++k) s.dirs[(size_t)k * p.n + i] = dirs[k];
    }
    s.pos[i] = pos;
    s.aux[i] = aux;
    s.step[i] = w[2];
    s.pid[i] = pid;
    if (!flg) return;
    // the last move of the path (move len - 2), which the traceback rule needs
    uint32_t last = 0;
    if constexpr (TB) {
        if (len >= 2u) {
            const uint32_t k = len - 2u;
            uint64_t dw = 0;
#pragma unroll
            for (int j = 0; j < 2 * W; ++j) dw |= dirs[j] & ((k >> 5) == (uint32_t)j ? ~0ull : 0ull);
            last = (uint32_t)(dw >> ((k & 31u) * 2u)) & 3u;
        }
    }
    flg[i] = (uint8_t)(record_legal<W, TB>(p, pos, pid, vis, last) << 2);
}

}  // namespace sparc
