// sparc_observe.hpp — observation planes of state records (device code): M records -> the
// 'visited' and 'agent_location' planes of obs['base'] (_get_obs, SPaRC_Gym.py:956-979) plus the
// puzzle index, the agent's (x, y) and the legal actions of every record, in one launch and without
// an env: the context supplies its tables, pitch and traceback mode only.
//
// Included by sparc_kernels.hip after the plane staging and writers it builds on (ObsWave /
// obs_write_as, ObsStream / obs_write_stream_as); bit for bit the planes are what k_obs_pack writes
// for an env that k_restore filled from the record.
//
//   One lane per record, 256-thread workgroups.  A record stores its visited board in plane bit
//   order (bit x * pitch + y), so a lane reads the record's first 16-B piece (pos, aux, step, pid)
//   and the W visited words behind it, and nothing else of it unless the legal byte is asked for
//   under traceback: then the one 32-bit word of the direction stack that holds the path's last
//   move (the only legal revisit is its reverse, SPaRC_Gym.py:1024-1051).
//   The record is validated (expand_record_ok, the conditions of k_restore) before anything is
//   indexed with it.  A record that fails is staged as an empty board without an agent, so its two
//   planes are all zero, gets puzzle 0xFFFFFFFF, loc (0, 0) and legal 0, and raises kErrSnapshot.
//   Each wave stages its 64 boards in LDS and writes each plane's run as whole 16-B nontemporal
//   pieces, one store instruction covering 1 KB of contiguous memory (obs_write_as; on multi-word
//   pools whose board bit IS the plane cell, dense output takes the bit streams of
//   obs_write_stream_as).  The element (1, 2 or 4 bytes) is a template parameter, the pattern of
//   "one" a launch argument.  With a stride the plane of record j starts at element j * stride of
//   each base (the two channels of a caller's [M][C][x][y] network input): obs_write_plane stores
//   the 16-B aligned pieces inside each plane whole and the cells at its ends singly, and nothing
//   is written between the planes.
//   The three scalars are coalesced stores of 4, 8 and 1 bytes per lane.
//   Written per record: 2 * XD * YD * sizeof(E) + 13 bytes; read: 16 + 8 W (+ 4).
//
// No namespace of its own: it lives where sparc_kernels.hip includes it, next to the helpers.
#pragma once
#include "sparc_expand.hpp"

struct ObserveOut {
    void* vis;            // [M] planes of XD * YD elements, `stride` elements apart; may be NULL
    void* agent;          // as vis; may be NULL
    uint32_t XD, YD;
    uint64_t stride;      // elements between the planes of consecutive records; 0: dense (XD * YD)
    uint32_t one;         // the element's bit pattern of 1
    uint32_t* puzzle;     // [M]; may be NULL
    int32_t* loc;         // [M][2] (x, y); may be NULL
    uint8_t* legal;       // [M] bits 0-3; may be NULL
};

// the agent "bit" of a refused record: no cell's, and not kObsNone either (the padding cells' entry)
constexpr uint32_t kObsNoAgent = 0xFFFEu;

// one wave's staging: the boards by lane (LUT path) or the two bit streams
template <int W>
__host__ __device__ constexpr size_t observe_buf_bytes() {
    return ((sizeof(ObsWave<W>) > sizeof(ObsStream<W>) ? sizeof(ObsWave<W>) : sizeof(ObsStream<W>)) + 15) / 16 * 16;
}

template <int W, bool TB, class E>
__global__ void __launch_bounds__(kSnapBlock) k_observe_rec(Params p, const uint4* __restrict__ rec, uint32_t M,
                                                            ObserveOut o) {
    using R = SnapRec<W, TB>;
    constexpr size_t kBuf = observe_buf_bytes<W>();
    __shared__ __attribute__((aligned(16))) uint8_t stage[(kSnapBlock / 64) * kBuf];
    __shared__ uint16_t lut[kObsCells];
    const uint32_t XY = o.XD * o.YD;
    const bool planes = o.vis || o.agent;                                             // block-uniform
    const bool stream = o.stride == 0 && obs_stream_ok<W>(p.pitch, o.XD, o.YD);       // block-uniform
    if (planes) {
        if (stream) {   // the bit streams start at 0
            for (uint32_t k = threadIdx.x; k < sizeof(stage) / 4; k += kSnapBlock) reinterpret_cast<uint32_t*>(stage)[k] = 0u;
        } else {
            obs_build_lut(lut, o.XD, o.YD, p.pitch, W, threadIdx.x, kSnapBlock);
        }
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t j0 = blockIdx.x * kSnapBlock + wave * 64u, j = j0 + lane;
    if (j0 >= M) return;                                                              // wave-uniform
    const uint32_t cnt = M - j0 < 64u ? M - j0 : 64u;
    uint64_t v[W];
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = 0;
    uint32_t ab = kObsNoAgent;
    bool ok = false;
    if (j < M) {
        const uint4* pc = rec + (size_t)j * R::kPieces;
        const uint4 head = pc[0];
        const uint32_t pos = head.x, pid = head.w;
        const uint32_t x = pos & 0xFFu, y = (pos >> 8) & 0xFFu, len = (pos >> 16) & 0xFFu;
        ok = expand_record_ok(p.tab, pos, head.y, pid);
        uint32_t legal = 0;
        if (ok) {
            const uint2* pv = reinterpret_cast<const uint2*>(pc + 1);   // the visited words follow the scalars
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const uint2 h = pv[k];
                v[k] = h.x | ((uint64_t)h.y << 32);
            }
            ab = x * p.pitch + y;
            if (o.legal) {
                uint32_t last = 0;
                if constexpr (TB) {
                    if (len >= 2u) {   // move len - 2: 16 moves per 32-bit word of the stack
                        const uint32_t k = len - 2u, wi = (k >> 4) < 4u * W ? (k >> 4) : 4u * W - 1u;   // inside the record
                        last = (reinterpret_cast<const uint32_t*>(pc)[R::kDirs + wi] >> ((k & 15u) * 2u)) & 3u;
                    }
                }
                legal = record_legal<W, TB>(p, pos, pid, v, last);
            }
        } else {
            atomicOr(p.err, (int)kErrSnapshot);
        }
        if (o.puzzle) o.puzzle[j] = ok ? pid : 0xFFFFFFFFu;
        if (o.loc) reinterpret_cast<int2*>(o.loc)[j] = ok ? make_int2((int)x, (int)y) : make_int2(0, 0);
        if (o.legal) o.legal[j] = (uint8_t)legal;
    }
    if (!planes) return;
    uint8_t* bk = stage + wave * kBuf;
    E* vo = static_cast<E*>(o.vis);
    E* ao = static_cast<E*>(o.agent);
    if (stream) {
        ObsStream<W>* os = reinterpret_cast<ObsStream<W>*>(bk);
        obs_stage_stream<W>(os, lane, ok, v, ab, XY);
        wave_lds_fence();
        const size_t run = (size_t)j0 * XY;
        obs_write_stream_as<W, E>(os, lane, cnt, XY, vo ? vo + run : nullptr, ao ? ao + run : nullptr, o.one);
    } else {
        ObsWave<W>* ow = reinterpret_cast<ObsWave<W>*>(bk);
        obs_stage<W>(ow, lane, true, v, ab);
        wave_lds_fence();
        if (o.stride == 0) {
            const size_t run = (size_t)j0 * XY;
            obs_write_as<W, E, false>(ow, lut, lane, cnt, XY, vo ? vo + run : nullptr, ao ? ao + run : nullptr, o.one, 0);
        } else {
            const size_t run = (size_t)j0 * o.stride;
            obs_write_as<W, E, true>(ow, lut, lane, cnt, XY, vo ? vo + run : nullptr, ao ? ao + run : nullptr, o.one,
                                     (size_t)o.stride);
        }
    }
}
