// sparc_reach.hpp — target reachability and distance maps of state records (device code): for each
// of M records, whether the free lattice points still connect the agent to the target, how far the
// target is through each action, the size of the target's component and (optionally) the distance
// plane, in one launch and without an env: the context supplies its puzzle tables and pitch only
// (no reset, no rule tables, not the traceback mode).  The reference has no counterpart; a forward
// move is _get_legal_actions (SPaRC_Gym.py:1024-1051) without the traceback revisit.
//
// Definition (integers only).  F = the puzzle's open points (no gap, inside its lattice) that the
// record has not visited; the agent's own point is visited, so never free.  C = the 4-connected
// component of F that holds the target (empty when the target is visited, which covers the agent
// standing on it), D(p) = breadth-first distance from p in C to the target.
//   action_dist[a]  1 + D(n_a) when the neighbour n_a in direction a lies in the lattice and in C,
//                   else 255: exact for the child (a shortest path from n_a never returns to n_a)
//   live            bit a set iff action_dist[a] != 255
//   dist            0 on the target, else min(action_dist), 255 when there is none
//   size            |C| (at most 254: kMaxPathPoints open points, one of them the agent's)
//   plane[x][y]     D on C, 255 elsewhere (cells outside the puzzle's lattice included)
//
// One lane per record, 256-lane workgroups; a lane reads the record's first 16-B piece and the W
// visited words behind it (as k_observe_rec), and validates it (expand_record_ok) before anything
// is indexed with it.  A record that fails is flooded on an empty board: every output 255 / 0, the
// plane 255, kErrSnapshot raised.
//
// The flood (reach_flood) runs from the target: R <- target & F, each trip R <- R | (dilate(R) & F).
// Before trip k dilates, the points that entered R last (D == k) are looked at: a neighbour of the
// agent among them gets action_dist k + 1, and the visitor (the plane writer) sees them.  All 64
// lanes run every trip (a finished lane's trip changes nothing), and the wave leaves on a ballot
// when no lane's R grew; 255 trips bound the loop whatever the record holds.
//   W = 1: the padded board.  The guard column and guard row are never open, so plain shifts by 1
//          and by the pitch suffice; past the last row of a board that fills the word an x-step
//          falls off it.
//   W > 1: the pitch may equal y_max, where a y-step from a row's end would land in the next row:
//          the shifts by 1 are masked with the first- / last-column masks of the pitch (ReachGeom,
//          built by the host from the pitch alone, NOT the rule rows: no sparc_load_rules needed).
//          Shifts cross the 64-bit words; a pitch of 64 or more moves whole words first.
// The plane is a byte per cell.  Each wave keeps its 64 planes in LDS, [64][XD * YD] bytes preset to
// 255 (dynamic LDS, 256 * XD * YD <= 64 KiB per workgroup, none without the plane): that IS the
// wave's contiguous run of the output, so after the flood it is copied out as whole 16-B
// nontemporal pieces.  A lane writes k at the cells of its trip-k points.
// Read per record: 16 + 8 W bytes; written: 7 (+ XD * YD).
//
// No namespace of its own: it lives where sparc_kernels.hip includes it, next to the helpers.
#pragma once
#include "sparc_expand.hpp"

constexpr uint32_t kReachNone = 255u;   // SPARC_REACH_NONE
constexpr uint32_t kReachTrips = 255u;  // D <= 253, so the trip that finds nothing new comes earlier

// what the flood needs of the geometry besides the pitch; uniform per launch (reach_geom, host)
struct ReachGeom {
    uint64_t nfirst[4];   // bit b set iff b % pitch != 0          (a +y step cannot land there from y - 1)
    uint64_t nlast[4];    // bit b set iff b % pitch != pitch - 1  (a -y step cannot land there from y + 1)
    uint32_t magic;       // ceil(65536 / pitch): b / pitch == (b * magic) >> 16 for b < 256
};

struct ReachOut {
    uint8_t* dist;    // [M]; may be NULL
    uint8_t* adist;   // [M][4]; may be NULL
    uint8_t* live;    // [M]; may be NULL
    uint8_t* size;    // [M]; may be NULL
    uint8_t* plane;   // [M][XD * YD]; may be NULL
    uint32_t XD, YD;
};

// toward higher / lower bit indices by s (0 < s < 64 W), bits past the board dropped
template <int W>
__device__ __forceinline__ void reach_shl(const uint64_t (&v)[W], uint32_t s, uint64_t (&r)[W]) {
    const uint32_t ws = s >> 6, bs = s & 63u;   // launch-uniform
#pragma unroll
    for (int k = W - 1; k >= 0; --k) {
        uint64_t hi = 0, lo = 0;                // words k - ws and k - ws - 1 of v
#pragma unroll
        for (int j = 0; j < W; ++j) {
            hi |= (uint32_t)j + ws == (uint32_t)k ? v[j] : 0ull;
            lo |= (uint32_t)j + ws + 1u == (uint32_t)k ? v[j] : 0ull;
        }
        r[k] = (hi << bs) | ((lo >> 1) >> (63u - bs));
    }
}
template <int W>
__device__ __forceinline__ void reach_shr(const uint64_t (&v)[W], uint32_t s, uint64_t (&r)[W]) {
    const uint32_t ws = s >> 6, bs = s & 63u;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        uint64_t lo = 0, hi = 0;                // words k + ws and k + ws + 1 of v
#pragma unroll
        for (int j = 0; j < W; ++j) {
            lo |= (uint32_t)j == (uint32_t)k + ws ? v[j] : 0ull;
            hi |= (uint32_t)j == (uint32_t)k + ws + 1u ? v[j] : 0ull;
        }
        r[k] = (lo >> bs) | ((hi << 1) << (63u - bs));
    }
}

// the points one step from r, on the whole board (the caller masks with F)
template <int W>
__device__ __forceinline__ void reach_dilate(const uint64_t (&r)[W], uint32_t P, const ReachGeom& g, uint64_t (&n)[W]) {
    if constexpr (W == 1) {
        n[0] = (r[0] << 1) | (r[0] >> 1) | (r[0] << P) | (r[0] >> P);   // P <= 15; guards are never free
    } else {
        uint64_t a[W], b[W];
        if (P < 64u) {   // launch-uniform: the shifts cross one word boundary at most
#pragma unroll
            for (int k = 0; k < W; ++k) {
                a[k] = (r[k] << P) | (k ? r[k - 1] >> (64u - P) : 0ull);
                b[k] = (r[k] >> P) | (k + 1 < W ? r[k + 1] << (64u - P) : 0ull);
            }
        } else {
            reach_shl<W>(r, P, a);
            reach_shr<W>(r, P, b);
        }
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const uint64_t up = (r[k] << 1) | (k ? r[k - 1] >> 63 : 0ull);
            const uint64_t dn = (r[k] >> 1) | (k + 1 < W ? r[k + 1] << 63 : 0ull);
            n[k] = a[k] | b[k] | (up & g.nfirst[k]) | (dn & g.nlast[k]);
        }
    }
}

// The flood of one record per lane; every lane of the wave must call it (the loop leaves on a
// ballot), a lane without a record passes an empty `free`.
//   free    F: open & ~visited                       tbit  the target's bit
//   nb      the board bit of the neighbour in each direction (any value where !((nbv >> a) & 1))
//   nbv     bit a set iff that neighbour lies in the puzzle's lattice
//   R       out: the target component C
//   ad      out: action_dist, byte a (255: not in C)
//   visit(k, pts): the points at distance k, for k = 0, 1, .. while any lane of the wave has some
template <int W, class Visit>
__device__ __forceinline__ void reach_flood(const uint64_t (&free)[W], uint32_t tbit, const uint32_t (&nb)[4],
                                            uint32_t nbv, uint32_t P, const ReachGeom& g, uint64_t (&R)[W],
                                            uint32_t& ad, Visit&& visit) {
    uint64_t nw[W], nbm[W];   // the points that entered R last; the agent's neighbours
#pragma unroll
    for (int k = 0; k < W; ++k) R[k] = 0, nbm[k] = 0;
    sparc::bb_set<W>(R, tbit);
#pragma unroll
    for (uint32_t a = 0; a < 4; ++a) {
        uint64_t one[W];
#pragma unroll
        for (int k = 0; k < W; ++k) one[k] = 0;
        sparc::bb_set<W>(one, nb[a]);
#pragma unroll
        for (int k = 0; k < W; ++k) nbm[k] |= ((nbv >> a) & 1u) ? one[k] : 0ull;
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
        R[k] &= free[k];
        nw[k] = R[k];
    }
    ad = 0xFFFFFFFFu;
    for (uint32_t trip = 0; trip < kReachTrips; ++trip) {
        uint64_t hit = 0, grew = 0;
#pragma unroll
        for (int k = 0; k < W; ++k) hit |= nw[k] & nbm[k];
        if (hit) {   // a neighbour of the agent at distance `trip`
#pragma unroll
            for (uint32_t a = 0; a < 4; ++a) {
                const bool in = ((nbv >> a) & 1u) && sparc::bb_test<W>(nw, nb[a]);
                ad = in ? (ad & ~(0xFFu << (8u * a))) | ((trip + 1u) << (8u * a)) : ad;
            }
        }
        visit(trip, nw);
        uint64_t n[W];
        reach_dilate<W>(R, P, g, n);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            nw[k] = n[k] & free[k] & ~R[k];
            R[k] |= nw[k];
            grew |= nw[k];
        }
        if (__builtin_amdgcn_ballot_w64(grew != 0) == 0) break;   // wave-uniform
    }
}

// `plane` dynamic LDS: (kSnapBlock / 64) tiles of 64 * XD * YD bytes when o.plane, else none
template <int W, bool TB>
__global__ void __launch_bounds__(kSnapBlock) k_reach_rec(Params p, const uint4* __restrict__ rec, uint32_t M,
                                                          ReachOut o, ReachGeom g) {
    using R = SnapRec<W, TB>;
    extern __shared__ __attribute__((aligned(16))) uint8_t reach_tiles[];
    const uint32_t XY = o.XD * o.YD;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t j0 = blockIdx.x * kSnapBlock + wave * 64u, j = j0 + lane;
    if (j0 >= M) return;                                                              // wave-uniform
    const uint32_t cnt = M - j0 < 64u ? M - j0 : 64u;
    uint8_t* const tile = reach_tiles + (size_t)wave * 64u * XY;   // this wave's planes; 64 * XY is a multiple of 16
    if (o.plane) {
        for (uint32_t k = lane; k < 4u * XY; k += 64u) reinterpret_cast<u32x4*>(tile)[k] = u32x4{~0u, ~0u, ~0u, ~0u};
        wave_lds_fence();
    }
    uint64_t fr[W];
#pragma unroll
    for (int k = 0; k < W; ++k) fr[k] = 0;
    uint32_t tbit = 0, nbv = 0, nb[4] = {0u, 0u, 0u, 0u};
    bool ok = false, on_target = false;
    if (j < M) {
        const uint4* pc = rec + (size_t)j * R::kPieces;
        const uint4 head = pc[0];
        const uint32_t pos = head.x, pid = head.w;
        ok = expand_record_ok(p.tab, pos, head.y, pid);
        if (ok) {
            const uint2* pv = reinterpret_cast<const uint2*>(pc + 1);   // the visited words follow the scalars
            const uint4 inf = p.tab.info[pid];
            const uint32_t X = inf.x & 0xFFu, Y = (inf.x >> 8) & 0xFFu, tx = inf.y & 0xFFu, ty = (inf.y >> 8) & 0xFFu;
            const uint32_t x = pos & 0xFFu, y = (pos >> 8) & 0xFFu, b = x * p.pitch + y;
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const uint2 h = pv[k];
                fr[k] = p.tab.open[(size_t)pid * W + k] & ~(h.x | ((uint64_t)h.y << 32));
            }
            tbit = tx * p.pitch + ty;
            on_target = x == tx && y == ty;
            nbv = (uint32_t)(x + 1u < X) | ((uint32_t)(y > 0u) << 1) | ((uint32_t)(x > 0u) << 2) | ((uint32_t)(y + 1u < Y) << 3);
            nb[0] = b + p.pitch, nb[1] = b - 1u, nb[2] = b - p.pitch, nb[3] = b + 1u;
#pragma unroll
            for (int a = 0; a < 4; ++a) nb[a] = ((nbv >> a) & 1u) ? nb[a] : 0u;
        } else {
            atomicOr(p.err, (int)kErrSnapshot);
        }
    }
    uint64_t C[W];
    uint32_t ad;
    uint8_t* const mine = tile + lane * XY;
    const bool plane = o.plane != nullptr;   // block-uniform
    reach_flood<W>(fr, tbit, nb, nbv, p.pitch, g, C, ad, [&](uint32_t k, const uint64_t (&pts)[W]) {
        if (!plane) return;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            uint64_t t = pts[w];
            while (t) {   // C lies in the puzzle's lattice, so x < XD and y < YD
                const uint32_t bit = 64u * w + (uint32_t)__builtin_ctzll(t);
                const uint32_t x = (bit * g.magic) >> 16, y = bit - x * p.pitch;
                if (x < o.XD && y < o.YD) mine[x * o.YD + y] = (uint8_t)k;
                t &= t - 1;
            }
        }
    });
    if (j < M) {
        uint32_t sz = 0, lv = 0, d = kReachNone;
#pragma unroll
        for (int k = 0; k < W; ++k) sz += (uint32_t)__builtin_popcountll(C[k]);
#pragma unroll
        for (uint32_t a = 0; a < 4; ++a) {
            const uint32_t da = (ad >> (8u * a)) & 0xFFu;
            lv |= (uint32_t)(da != kReachNone) << a;
            d = da < d ? da : d;
        }
        if (on_target) d = 0;
        if (o.dist) o.dist[j] = (uint8_t)d;
        if (o.live) o.live[j] = (uint8_t)lv;
        if (o.size) o.size[j] = (uint8_t)sz;
        if (o.adist) {
            if ((reinterpret_cast<uintptr_t>(o.adist) & 3u) == 0) {   // uniform
                reinterpret_cast<uint32_t*>(o.adist)[j] = ad;
            } else {
#pragma unroll
                for (uint32_t a = 0; a < 4; ++a) o.adist[4u * (size_t)j + a] = (uint8_t)(ad >> (8u * a));
            }
        }
    }
    if (!plane) return;
    wave_lds_fence();
    // the wave's planes [0, cnt) are one run of cnt * XY bytes of the output
    uint8_t* const out = o.plane + (size_t)j0 * XY;
    const uint32_t total = cnt * XY;
    const uint32_t whole = (reinterpret_cast<uintptr_t>(out) & 15u) == 0 ? total & ~15u : 0u;   // bytes stored as pieces
    for (uint32_t f = 16u * lane; f < whole; f += 1024u)
        __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(tile + f), reinterpret_cast<u32x4*>(out + f));
    for (uint32_t f = whole + lane; f < total; f += 64u) out[f] = tile[f];
}
