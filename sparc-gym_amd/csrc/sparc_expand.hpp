// sparc_expand.hpp — one-ply expansion of state records (device code): the successor function a
// tree search needs, M parent records -> 4M child records + the steps' reward codes and flags.
//
// Child (j, a) is the record k_snapshot writes for an env that k_restore filled from record j
// and k_step stepped once with action a (SPaRC_Gym.py:1111-1238), in one launch and without an
// env: the context supplies the tables, pitch, max_steps and autoreset mode only.
//
//   One lane per child: thread t of a 256-thread workgroup handles parent t >> 2 with action
//   t & 3.  The four lanes of a parent read the same record (one or two cache lines).
//   The step is the project's own: the lane puts the parent's fields into ITS slot of a 256-slot
//   SoA in LDS, and a copy of Params whose State pointers and n describe that SoA lets
//   Env::load / Env::advance / Env::store run on it exactly as k_step runs them on the global
//   SoA (the W = 1 specialisation's canonical stored form included).  A lane reads and writes
//   its own slot only, so no barrier is needed around the step.
//   The stepped slot is read back into registers, and then the same LDS holds the workgroup's
//   256 child records, one contiguous run of the output, stored as whole 16-B pieces (piece
//   k*64 + lane of each wave's run) as k_snapshot does.  A record is at least as large as a
//   slot (16 + 8W (+ 16W) bytes, padded), so LDS is 256 * record_bytes: 12 KB (W = 1,
//   traceback) to 28 KB (W = 4, traceback).
//   A wave's 64 reward codes and its 64 flag bytes are 64 contiguous bytes each.
//
// A parent record is checked before anything is indexed with it, with the conditions of
// k_restore (its own copy here: k_restore is left as it is).  A parent that fails gets four
// zeroed children (len 0, which no restore or expand accepts), code 0, flags 0, parent flags 0,
// and raises kErrSnapshot.
#pragma once
#include "sparc_snapshot.hpp"

namespace sparc {

// the conditions k_restore applies to a record: pid < P, x < x_size, y < y_size, 1 <= len <= the
// lattice's points, the trie node below the puzzle's node count (0 on a puzzle without a root)
__device__ __forceinline__ bool expand_record_ok(const Table& tab, uint32_t pos, uint32_t aux, uint32_t pid) {
    if (pid >= tab.num_puzzles) return false;
    const uint32_t x = pos & 0xFFu, y = (pos >> 8) & 0xFFu, len = (pos >> 16) & 0xFFu;
    const uint4 inf = tab.info[pid];
    const uint32_t X = inf.x & 0xFFu, Y = (inf.x >> 8) & 0xFFu;
    const uint32_t nodes = ((inf.y >> 16) & 2u) ? (inf.w & 0xFFFFu) : 1u;
    return x < X && y < Y && len >= 1u && len <= X * Y && (aux & 0xFFFFu) < nodes;
}

// Child 4j + a <- step(record j, action a) for j < M (M4 = 4M < 2^31).  rew, flg [4M] and
// pflg [M] (the parent's legal actions in bits 2-5, as k_restore's flags) may be NULL.
template <int W, bool TB>
__global__ void __launch_bounds__(kSnapBlock) k_expand(Params p, const uint4* __restrict__ rec, uint32_t M4,
                                                       uint4* __restrict__ out, int8_t* __restrict__ rew,
                                                       uint8_t* __restrict__ flg, uint8_t* __restrict__ pflg) {
    using R = SnapRec<W, TB>;
    constexpr int kD = TB ? 2 * W : 0;                       // direction-stack words of a slot
    static_assert((W + kD) * 8 + 16 <= R::kBytes, "an SoA slot fits in a record");
    __shared__ uint4 stage[kSnapBlock * R::kPieces];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t j = blockIdx.x * kSnapBlock + t;
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
    uint32_t w[R::kWords];
#pragma unroll
    for (int k = 0; k < R::kWords; ++k) w[k] = 0;
    if (j < M4) {
        const uint32_t a = j & 3u, par = j >> 2;
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
        int code = 0;
        uint32_t f = 0, pf = 0;
        if (expand_record_ok(p.tab, r[0], r[1], r[3])) {
            const State& s = q.st;
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
            const PuzzleSrc<W> src{p.tab.info, p.tab.root, p.tab.open, p.tab.init, p.tab.row1};
            Env<W, TB> e;
            e.load(q, src, t);
            pf = e.legal << 2;
            code = e.advance(q, src, a, f);
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
        } else if (a == 0) {
            atomicOr(p.err, (int)kErrSnapshot);
        }
        if (rew) rew[j] = (int8_t)code;
        if (flg) flg[j] = (uint8_t)f;
        if (a == 0 && pflg) pflg[par] = (uint8_t)pf;
    }
    __syncthreads();   // every slot has been read back: the LDS now takes the records
    uint4* wl = stage + wave * 64u * R::kPieces;
#pragma unroll
    for (int k = 0; k < R::kPieces; ++k)
        wl[lane * R::kPieces + k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    __syncthreads();
    // this wave's children are one contiguous run of the output: piece k*64 + lane per store
    const uint32_t j0 = blockIdx.x * kSnapBlock + wave * 64u;
    const uint32_t cnt = j0 < M4 ? (M4 - j0 < 64u ? M4 - j0 : 64u) : 0u;
    uint4* run = out + (size_t)j0 * R::kPieces;
#pragma unroll
    for (int k = 0; k < R::kPieces; ++k) {
        const uint32_t qi = (uint32_t)k * 64u + lane;
        if (qi < cnt * R::kPieces) run[qi] = wl[qi];
    }
}

}  // namespace sparc
