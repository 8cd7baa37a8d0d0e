// sparc_mcts.hpp — UCT tree search of state records (device code): one search tree per record, kept
// in caller-owned memory between launches, grown by `sims` simulations per launch and without an
// env.  The context supplies the tables, pitch and max_steps only.  The top of the search stack:
// the tree policy picks among the forward moves of sparc_dfs.hpp, the value of a new node is one
// legal-move playout of sparc_playout.hpp.
//
//   One lane per record (root), 256-lane workgroups; one lane owns one tree, so there are no
//   atomics.  As in k_playout the lane puts the root's fields into ITS slot of a 256-slot SoA in
//   LDS; Env::load reads them at the start of every simulation, and through a simulation the Env
//   stays in registers.  The step is the project's own: Env::advance, one real step()
//   (SPaRC_Gym.py:1111-1238) with its reward code and flags.
//
//   The tree of root j is nodes[j][0 .. count[j]) of an arena [M][cap] of 64-byte nodes; node 0 is
//   the root.  The tree policy reads one node (one 64-B line) per level and never its children:
//     w0      parent | action that entered the node << 28 | kind << 30 (0 inner, 1 the step
//             terminated, 1192, 2 it truncated, 1134 / 1195, 3 live without a forward move)
//     w1-3    visits, wins (simulations through the node whose last reward code was +100), losses
//             (-100)
//     w4-7    child[a]: 0 not yet tried, 0xFFFFFFFF not a child, else the node's index
//     w8-11   n[a]: the visits of that child;  w12-15  wins[a]: its wins
//   The children of an inner node are its legal actions (_get_legal_actions, 1024-1051) without
//   the traceback pop (pop_bit): dfs_children.  A node of another kind has none.
//
//   One trip of the loop is at most one step of each lane, whatever the lane is doing, so the
//   lanes of a wave meet in one Env::advance:
//     in the tree, at an inner node with an untried child: the lowest untried action, the step,
//       and the new node is appended (FULL when the arena has no room: the simulation is dropped
//       before anything of it is written); an inner new node starts the rollout;
//     in the tree, every child tried: the first action that maximises
//       wins[a] / n[a] + ep[min(visits, T-1)] * ec[min(n[a], T-1)] under strict >, each operation
//       rounded to nearest by its own instruction (mcts_score: nothing is contracted, so a
//       float32 model reproduces every choice), the step, and the child is
//       entered; a child of kind != 0 ends the simulation;
//     in the rollout: k_playout's loop, a = uint_rand_pick(seed, id0 + j * 2^32 + s, t, mask) for
//       rollout step t < L, s the root's visits before the simulation; SPARC_PLAYOUT_FORWARD
//       clears the pop; it ends with the step that ends the episode, after L steps, or on a dead
//       end.
//   A finished simulation is backed up along the parent links, from the deepest tree node to the
//   root: visits, wins / losses by the last step's reward code, and n[a], wins[a] of the edge in
//   each parent.  A +100 ending with fewer steps from the root than win_steps[j] replaces the
//   winner: Env::store into the slot, the record read back from it (byte for byte what restore of
//   the root, those steps and snapshot give), and the root put into the slot again.
//   A wave leaves the loop when none of its lanes is live.
//
// A root record is checked with expand_record_ok before anything is indexed with it.  Of a tree
// that is continued nothing is trusted: count <= cap, and on the way down a child index must lie
// in (node, count) and the child's parent link and action must point back, so the walk down only
// rises through the arena, the walk up only falls, and no byte outside the root's cap nodes is
// read or written.  A root that fails is INVALID, raises kErrSnapshot and leaves the others alone.
#pragma once
#include "sparc_playout.hpp"

namespace sparc {

// status (sparc_gym_amd.h SPARC_MCTS_*)
constexpr uint32_t kMctsInvalid = 0, kMctsDone = 1, kMctsFull = 2, kMctsPending = 3, kMctsDeadEnd = 4;
constexpr uint32_t kMctsNone = 0xFFFFFFFFu;          // child[a]: not a child
constexpr uint32_t kMctsParentMask = 0x0FFFFFFFu;    // w0 bits 0-27
constexpr uint32_t kMctsNodePieces = 4;              // 16-B pieces of a node

struct MctsOut {
    uint8_t* __restrict__ status;       // [M]
    uint32_t* __restrict__ sims_done;   // [M] simulations of this call
    uint4* __restrict__ win_rec;        // [M] records, in/out
    uint32_t* __restrict__ win_steps;   // [M] in/out, 0xFFFFFFFF: no winner yet
};

// the forward moves of the state: its legal actions without the traceback pop (dfs_children, for
// either traceback setting)
template <int W, bool TB>
__device__ __forceinline__ uint32_t mcts_children(const Env<W, TB>& e) {
    return e.legal & ~pop_bit<W, TB>(e) & 15u;
}

// record `pc` into slot t of the workgroup's SoA, as k_playout puts it there; false (nothing
// written) if the record fails expand_record_ok
template <int W, bool TB>
__device__ __forceinline__ bool mcts_put_root(const Params& p, const State& s, const uint4* __restrict__ pc,
                                              uint32_t t) {
    using R = SnapRec<W, TB>;
    constexpr int kD = TB ? 2 * W : 0;
    uint32_t r[R::kWords];
#pragma unroll
    for (int k = 0; k < R::kPieces; ++k) {
        const uint4 v = pc[k];
        r[4 * k] = v.x;
        r[4 * k + 1] = v.y;
        r[4 * k + 2] = v.z;
        r[4 * k + 3] = v.w;
    }
    if (!expand_record_ok(p.tab, r[0], r[1], r[3])) return false;
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
    return true;
}

// the record held by slot t of the workgroup's SoA, to dst (k_playout's final record)
template <int W, bool TB>
__device__ __forceinline__ void mcts_slot_record(const State& s, uint32_t t, uint4* __restrict__ dst) {
    using R = SnapRec<W, TB>;
    constexpr int kD = TB ? 2 * W : 0;
    uint32_t w[R::kWords];
#pragma unroll
    for (int k = 0; k < R::kWords; ++k) w[k] = 0;
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
#pragma unroll
    for (int k = 0; k < kD; ++k) {
        const uint64_t v = s.dirs[k * kSnapBlock + t];
        w[R::kDirs + 2 * k] = (uint32_t)v;
        w[R::kDirs + 2 * k + 1] = (uint32_t)(v >> 32);
    }
#pragma unroll
    for (int k = 0; k < R::kPieces; ++k) dst[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

// the tree policy's score of a child: wins / n + pe * ce, three float32 operations with one rounding
// to nearest each.  Written with the plain operators under a contract(off) pragma, NOT with
// __fmul_rn / __fadd_rn: HIP defines those as inline functions of the operators, compiled under
// hipcc's default fp-contract=fast, so after inlining the backend still fuses them into one
// v_fmac_f32, which rounds once instead of twice (seen in the ISA).  With the pragma the ISA shows
// v_mul_f32 and v_add_f32 after the division's v_div_fixup_f32 (the correctly rounded division,
// hipcc's default for a float `/`).
__device__ __forceinline__ float mcts_score(uint32_t wins, uint32_t n, float pe, float ce) {
#pragma clang fp contract(off)
    const float mean = (float)wins / (float)n;
    const float bonus = pe * ce;
    return mean + bonus;
}

// a new node: entered from `parent` by action a, of kind `kind`, with the forward moves `moves`
__device__ __forceinline__ void mcts_new_node(uint4* node, uint32_t parent, uint32_t a, uint32_t kind,
                                              uint32_t moves) {
    const uint32_t m = kind == 0u ? moves : 0u;
    node[0] = make_uint4(parent | (a << 28) | (kind << 30), 0u, 0u, 0u);
    node[1] = make_uint4((m & 1u) ? 0u : kMctsNone, (m & 2u) ? 0u : kMctsNone, (m & 4u) ? 0u : kMctsNone,
                         (m & 8u) ? 0u : kMctsNone);
    node[2] = make_uint4(0u, 0u, 0u, 0u);
    node[3] = make_uint4(0u, 0u, 0u, 0u);
}

// Root j < M (M < 2^31): `sims` simulations on nodes[j][0 .. cap), count[j] of them in use (0: a
// fresh tree).  See the head of this file and sparc_mcts_device (sparc_gym_amd.h).  1 <= L, 2 <= T,
// 1 <= cap <= 2^24.
template <int W, bool TB>
__global__ void __launch_bounds__(kSnapBlock) k_mcts(Params p, const uint4* __restrict__ rec, uint32_t M,
                                                     uint32_t sims, uint32_t L, uint64_t seed, uint64_t id0,
                                                     uint32_t pflags, const float* __restrict__ ep,
                                                     const float* __restrict__ ec, uint32_t T, uint32_t cap,
                                                     uint4* nodes, uint32_t* __restrict__ count, MctsOut o) {
    using R = SnapRec<W, TB>;
    constexpr int kD = TB ? 2 * W : 0;                       // direction-stack words of a slot
    static_assert((W + kD) * 8 + 16 <= R::kBytes, "an SoA slot fits in a record");
    __shared__ uint4 stage[kSnapBlock * R::kPieces];
    const uint32_t t = threadIdx.x;
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
    q.autoreset = 0;   // a simulation stops at the done step: no step ever starts from a pending state
    const State& s = q.st;
    const PuzzleSrc<W> src{p.tab.info, p.tab.root, p.tab.open, p.tab.init, p.tab.row1};
    const uint4* const root = rec + (size_t)(in ? j : 0u) * R::kPieces;
    uint4* const tree = nodes + (size_t)(in ? j : 0u) * cap * kMctsNodePieces;
    Env<W, TB> e;
    uint32_t status = kMctsInvalid, cnt = 0, ws = 0xFFFFFFFFu, done = 0, visits0 = 0;
    bool live = false, started = false;
    if (in) {
        cnt = count[j];
        ws = o.win_steps[j];
        if (cnt > cap || !mcts_put_root<W, TB>(p, s, root, t)) {
            atomicOr(p.err, (int)kErrSnapshot);
        } else {
            e.load(q, src, t);
            const uint32_t moves = mcts_children<W, TB>(e);
            if (e.pending) {
                status = kMctsPending;
            } else if (moves == 0u) {
                status = kMctsDeadEnd;
            } else {
                if (cnt == 0u) {                              // a fresh tree
                    mcts_new_node(tree, 0u, 0u, 0u, moves);
                    cnt = 1;
                }
                started = true;
                visits0 = tree[0].y;
                live = visits0 != 0xFFFFFFFFu;
                if (!live) status = kMctsFull;
            }
        }
    }
    const bool fwd_only = TB && (pflags & kPlayoutForward);
    const uint64_t idj = id0 + ((uint64_t)j << 32);
    uint32_t node = 0, steps = 0, rt = 0;
    bool roll = false;
    int code = 0;
    for (;;) {
        if (__ballot(live) == 0ull) break;
        if (live) {
            // what this trip does: at most one step with action a
            uint32_t a = 0, child = 0;
            bool go = false, expand = false, finish = false, bad = false, full = false;
            if (!roll) {
                const uint4 hd = tree[(size_t)node * kMctsNodePieces];
                const uint4 ch = tree[(size_t)node * kMctsNodePieces + 1];
                const uint32_t untried = (uint32_t)(ch.x == 0u) | ((uint32_t)(ch.y == 0u) << 1) |
                                         ((uint32_t)(ch.z == 0u) << 2) | ((uint32_t)(ch.w == 0u) << 3);
                if (untried != 0u) {
                    if (cnt >= cap) {
                        full = true;
                    } else {
                        a = (uint32_t)__builtin_ctz(untried);
                        expand = go = true;
                    }
                } else {
                    const uint4 nv = tree[(size_t)node * kMctsNodePieces + 2];
                    const uint4 nw = tree[(size_t)node * kMctsNodePieces + 3];
                    const uint32_t cs[4] = {ch.x, ch.y, ch.z, ch.w}, ns[4] = {nv.x, nv.y, nv.z, nv.w},
                                   wn[4] = {nw.x, nw.y, nw.z, nw.w};
                    const float pe = ep[hd.y < T - 1u ? hd.y : T - 1u];
                    uint32_t best = 4;
                    float top = 0.0f;
#pragma unroll
                    for (uint32_t b = 0; b < 4; ++b) {
                        if (cs[b] != kMctsNone) {
                            const float x = mcts_score(wn[b], ns[b], pe, ec[ns[b] < T - 1u ? ns[b] : T - 1u]);
                            if (best == 4u || x > top) {
                                best = b;
                                top = x;
                                child = cs[b];
                            }
                        }
                    }
                    a = best;
                    // an inner node has a child, and a child lies above its parent and inside the tree
                    if (best == 4u || child <= node || child >= cnt) bad = true;
                    else go = true;
                }
            } else {
                uint32_t mask = e.legal;
                if (fwd_only) mask &= ~pop_bit<W, TB>(e);
                if (mask == 0u && e.legal != 0u) {
                    finish = true;                            // a dead end: the last step's code stands
                } else {
                    a = uint_rand_pick(seed, idj + visits0, rt, mask);
                    go = true;
                }
            }
            if (go) {
                uint32_t f = 0;
                code = e.advance(q, src, a, f);
                steps += 1u;
                if (roll) {
                    rt += 1u;
                    finish = (f & 3u) != 0u || rt >= L;
                } else if (expand) {
                    const uint32_t moves = mcts_children<W, TB>(e);
                    const uint32_t kind = (f & 1u) ? 1u : ((f & 2u) ? 2u : (moves == 0u ? 3u : 0u));
                    mcts_new_node(tree + (size_t)cnt * kMctsNodePieces, node, a, kind, moves);
                    reinterpret_cast<uint32_t*>(tree + (size_t)node * kMctsNodePieces + 1)[a] = cnt;
                    node = cnt;
                    cnt += 1u;
                    roll = kind == 0u;
                    rt = 0;
                    finish = !roll;
                } else {
                    const uint32_t w0 = tree[(size_t)child * kMctsNodePieces].x;
                    if ((w0 & kMctsParentMask) != node || ((w0 >> 28) & 3u) != a) {
                        bad = true;                           // the child does not point back
                    } else {
                        node = child;
                        finish = (w0 >> 30) != 0u;
                    }
                }
            }
            if (finish && !bad) {
                const uint32_t win = code == 100 ? 1u : 0u, loss = code == -100 ? 1u : 0u;
                if (win && steps < ws) {
                    e.store(q, src, t);
                    mcts_slot_record<W, TB>(s, t, o.win_rec + (size_t)j * R::kPieces);
                    ws = steps;
                    mcts_put_root<W, TB>(p, s, root, t);      // the slot is the root's again
                }
                // from the deepest tree node to the root: every link was checked on the way down
                for (uint32_t n = node;;) {
                    uint4 hd = tree[(size_t)n * kMctsNodePieces];
                    hd.y += 1u;
                    hd.z += win;
                    hd.w += loss;
                    tree[(size_t)n * kMctsNodePieces] = hd;
                    const uint32_t par = hd.x & kMctsParentMask, ea = (hd.x >> 28) & 3u;
                    if (n == 0u || par >= n) break;
                    uint32_t* const pw = reinterpret_cast<uint32_t*>(tree + (size_t)par * kMctsNodePieces + 2);
                    pw[ea] += 1u;
                    pw[4 + ea] += win;
                    n = par;
                }
                visits0 += 1u;
                done += 1u;
                if (done >= sims) {
                    live = false;
                    status = kMctsDone;
                } else if (visits0 == 0xFFFFFFFFu) {
                    live = false;
                    status = kMctsFull;
                } else {
                    e.load(q, src, t);
                    node = 0;
                    steps = 0;
                    roll = false;
                    code = 0;
                }
            }
            if (full) {
                live = false;
                status = kMctsFull;
            }
            if (bad) {
                live = false;
                status = kMctsInvalid;
                atomicOr(p.err, (int)kErrSnapshot);
            }
        }
    }
    if (in) {
        o.status[j] = (uint8_t)status;
        o.sims_done[j] = done;
        o.win_steps[j] = ws;
        if (started) count[j] = cnt;
    }
}

}  // namespace sparc
