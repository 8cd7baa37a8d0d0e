// sparc_dfs_prune.hpp — the pruned depth-first search of state records (device code): the walk of
// sparc_dfs.hpp (k_dfs) with another set of children per node, and nothing else changed.
//
// Definition (integers only).  With F, C, D, action_dist and live of a node's state as sparc_reach.hpp
// defines them (F: open and not visited, the agent's own point visited; C: the target's component),
// the children of a node, the root included, are
//   SPARC_DFS_PRUNE_REACH (1)     the forward moves a with live bit a set;
//   SPARC_DFS_PRUNE_DEADLINE (2)  (with REACH) of those, the ones with
//                                 node.step + action_dist[a] <= max_steps.
// Action order, pre-order, the real step() per entered child, leaf classes, the audit, undecided
// leaves and OVERFLOW, the cursor, first_sat, "k calls of budget B do the first k * B nodes of the
// (pruned) walk" and the byte-for-byte promise for every record written are those of sparc_dfs.hpp.
// A live root with no admissible child is one dead end, COMPLETE, with no node entered.
// Consequences (facts, pinned by the tests), for the same root and max_steps:
//   TARGETS, SATISFIED, LISTED, BOTH, UNDECIDED and first_sat equal the unpruned walk's: a path to the
//     target is self-avoiding, so each of its moves is live where it is made (and in time);
//   DEAD_ENDS is 0 below the root under REACH: an entered non-target node came through a live move, so
//     it has a neighbour in C one step nearer the target;
//   TRUNCATED is 0 under DEADLINE: that neighbour is reached in time, too.
// With both cuts the walk is the union of the prefixes of the target paths.
//
// The flood is reach_flood (sparc_reach.hpp), which leaves its loop on a ballot: k_dfs calls
// moves() under a wave-level ballot with every lane of the wave, whatever the lane is doing (walking,
// looking ahead after the budget, owing a leaf, finished, invalid, past M); a lane with nothing to
// ask passes an empty board, and the walk's own loop is left on a ballot only.
// A node's moves are asked for on the trip after the lane came to stand on it: after an entry
// (Env::advance) and after an undo (dfs_undo), on the state as those leave it.  So an undo costs a
// flood too (recomputed, no per-lane stack of masks): the flood is paid per wave and trip, not per
// lane, and in a wave of 64 walks at unrelated phases nearly every trip has a lane that has just
// entered a node, so a stack of the parents' masks (127 B of LDS per lane, and at W = 4 a second
// workgroup per CU lost to it) would spare almost no flood.
//   W = 1: F is the Env's free board shifted back (fr >> pitch: fr is (open & ~visited) << pitch and
//          a move toggles single points of it).  Every neighbour counts as in the lattice: one that is
//          not is a guard bit, never free, or falls off the word, where bb_set / bb_test see nothing.
//   W > 1: open & ~vis with the lattice tests of k_reach_rec, and ReachGeom's column masks for a
//          pitch equal to y_max.
//
// No namespace of its own (sparc_reach.hpp): sparc_kernels.hip includes it behind sparc_reach.hpp.
#pragma once
#include "sparc_dfs.hpp"
#include "sparc_reach.hpp"

// the children policy of k_dfs for the pruned search (k_dfs<W, TABLE_ONLY, DfsLiveMoves>, a kernel argument); `mode` is SPARC_DFS_PRUNE_REACH (1) or
// REACH | DEADLINE (3), uniform per launch
struct DfsLiveMoves {
    static constexpr bool kPrune = true;
    ReachGeom g;
    uint32_t mode;

    // the admissible forward moves of the state in e as a 4-bit mask; wave-collective: every lane
    // calls it, the ones with ask = false get 0 (their e is not read into anything that matters)
    template <int W>
    __device__ __forceinline__ uint32_t moves(const sparc::Env<W, true>& e, const Params& p, bool ask) const {
        const uint32_t P = p.pitch;
        uint64_t fr[W];
        uint32_t tbit, nbv, nb[4];
        int64_t step;
        if constexpr (W == 1) {
            fr[0] = ask ? e.fr >> P : 0ull;
            tbit = e.tgt;
            nbv = 15u;
            nb[0] = e.e + P, nb[1] = e.e - 1u, nb[2] = e.e - P, nb[3] = e.e + 1u;
            step = (int64_t)e.step;
        } else {
#pragma unroll
            for (int k = 0; k < W; ++k) fr[k] = ask ? e.open[k] & ~e.vis[k] : 0ull;
            const uint32_t b = e.x * P + e.y;
            tbit = e.tx * P + e.ty;
            nbv = (uint32_t)(e.x + 1u < e.X) | ((uint32_t)(e.y > 0u) << 1) | ((uint32_t)(e.x > 0u) << 2) |
                  ((uint32_t)(e.y + 1u < e.Y) << 3);
            nb[0] = b + P, nb[1] = b - 1u, nb[2] = b - P, nb[3] = b + 1u;
            step = (int64_t)(int32_t)e.step;
        }
        nbv = ask ? nbv : 0u;
        tbit = ask ? tbit : 0u;
#pragma unroll
        for (int a = 0; a < 4; ++a) nb[a] = ((nbv >> a) & 1u) ? nb[a] : 0u;
        uint64_t C[W];
        uint32_t ad;
        reach_flood<W>(fr, tbit, nb, nbv, P, g, C, ad, [](uint32_t, const uint64_t (&)[W]) {});
        uint32_t m = 0;
#pragma unroll
        for (uint32_t a = 0; a < 4; ++a) {
            const uint32_t da = (ad >> (8u * a)) & 0xFFu;
            // 64-bit: step and max_steps are 32-bit and da goes up to 254, the sum must not wrap
            const bool in_time = !(mode & sparc::kDfsPruneDeadline) || step + (int64_t)da <= (int64_t)p.max_steps;
            m |= (uint32_t)(da != kReachNone && in_time) << a;
        }
        return ask ? m : 0u;
    }
};

// Before an unpruned walk (prune = 0) through sparc_dfs_pruned_device: a state word that is neither
// zero nor DONE and carries another mode loses its root length, which is how k_dfs, unchanged, knows
// a cursor it has to refuse (INVALID, DONE, kErrSnapshot; the other records unaffected).
__global__ void __launch_bounds__(kSnapBlock) k_dfs_mode0(uint32_t* __restrict__ state, uint32_t M) {
    const uint32_t j = blockIdx.x * kSnapBlock + threadIdx.x;
    if (j >= M) return;
    const uint32_t st = state[j];
    if (st != 0u && !(st & sparc::kDfsDone) && ((st >> sparc::kDfsModeShift) & 3u) != 0u) state[j] = st & ~0xFFu;
}
