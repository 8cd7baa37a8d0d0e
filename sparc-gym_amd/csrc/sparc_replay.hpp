// sparc_replay.hpp — replay of given action sequences from state records (device code): M
// sequences of up to L caller-supplied actions each, played in one launch and without an env,
// with the codes, flags, end state and (optionally) every state on the way.  The deterministic
// counterpart of k_playout: the reference's user steps the env with a model's proposed moves
// and reads the result (step, SPaRC_Gym.py:1111-1238); here that is one lane per proposal.  The
// context supplies the tables, pitch, max_steps and autoreset mode only.
//
//   One lane per sequence, kSnapBlock lanes per workgroup.  Sequence j starts from record j
//   (checked with expand_record_ok before anything is indexed with it, as k_playout) or from the
//   reset state of puzzle[j] (Env::reset, reset() 1057-1108: the state k_reset gives an env on
//   that puzzle with fresh planes), checked < num_puzzles.  A record's fields go into the lane's
//   slot of the workgroup's SoA in LDS and Env::load reads them; from then on the Env stays in
//   registers, and each step is Env::advance under the context's max_steps AND autoreset mode:
//   nothing is special-cased, as in k_expand.
//   Actions are [L][M] step-major, as k_playout's trace: one 64-byte load per wave and step.
//   The load of step t + 1's action is issued before step t's advance, so it is off the step's
//   dependency chain.  len[j] (NULL: L) actions belong to sequence j, clamped to L; there is no
//   sentinel action (255 is an illegal action like any value >= 4).
//   kReplayStopDone ends a sequence with the step that terminates or truncates (a start whose
//   pending bit is set takes no step); kReplayStopIllegal ends it BEFORE a step whose action is
//   not in the state's legal mask, and that action is not taken.
//   A wave leaves the loop when none of its lanes is live (__ballot); there is no block-wide
//   barrier inside the loop.
//   Env::store then writes the slot once, the slot is read back, and the same LDS holds the
//   workgroup's 256 final records, stored as whole 16-B pieces of each wave's contiguous run
//   (k_snapshot, k_expand, k_playout).  With no step taken that is the start record in canonical
//   stored form: this is how root records are made (L = 0).
//   STATES: the record after every step, [L][M], zeroed at and after the sequence's end: a
//   per-lane Env::store to the lane's own slot and 16-B stores from the lane (not the hot path;
//   the common instantiation compiles none of it).
//
// A start that fails its check gives end reason 0, zeroed outputs and raises kErrSnapshot.
#pragma once
#include "sparc_playout.hpp"

namespace sparc {

constexpr uint32_t kReplayStopDone = 1, kReplayStopIllegal = 2;   // SPARC_REPLAY_STOP_*

// end reasons (sparc_gym_amd.h SPARC_REPLAY_END_*)
constexpr uint32_t kRpInvalid = 0, kRpTerminated = 1, kRpTruncated = 2, kRpExhausted = 3, kRpIllegal = 4,
                   kRpPending = 5;

struct ReplayOut {
    int8_t* __restrict__ code;         // [M] the last step's reward code
    uint8_t* __restrict__ flags;       // [M] the last step's flag byte
    uint16_t* __restrict__ steps;      // [M] steps taken
    uint8_t* __restrict__ end;         // [M] end reason
    int32_t* __restrict__ ret;         // [M] sum of the reward codes
    uint16_t* __restrict__ bad;        // [M] index of the refused action, 0xFFFF: none
    int8_t* __restrict__ step_code;    // [L][M] code of step t, 0 at and after the end
    uint8_t* __restrict__ step_flags;  // [L][M] flag byte of step t, 0 at and after the end
    uint4* __restrict__ final_rec;     // [M] records
    uint4* __restrict__ states;        // [L][M] records (STATES only), zeroed at and after the end
};

// the lane's slot of the workgroup's SoA, as the words of a record
template <int W, bool TB>
__device__ __forceinline__ void replay_slot_words(const State& s, uint32_t t,
                                                  uint32_t (&w)[SnapRec<W, TB>::kWords]) {
    using R = SnapRec<W, TB>;
    constexpr int kD = TB ? 2 * W : 0;
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

// Sequence g < M (M < 2^31, L <= 65535): exactly one of rec / puzzle is non-NULL (host-checked).
template <int W, bool TB, bool STATES>
__global__ void __launch_bounds__(kSnapBlock) k_replay(Params p, const uint4* __restrict__ rec,
                                                       const uint32_t* __restrict__ puzzle, uint32_t M, uint32_t L,
                                                       const uint8_t* __restrict__ actions,
                                                       const uint32_t* __restrict__ len, uint32_t rflags, ReplayOut o) {
    using R = SnapRec<W, TB>;
    constexpr int kD = TB ? 2 * W : 0;                       // direction-stack words of a slot
    static_assert((W + kD) * 8 + 16 <= R::kBytes, "an SoA slot fits in a record");
    __shared__ uint4 stage[kSnapBlock * R::kPieces];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t g = blockIdx.x * kSnapBlock + t;
    const bool in = g < M;
    // the workgroup's SoA in LDS, seen through Params as Env::load / store see the global one;
    // the context's autoreset mode stays as it is
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
    const State& s = q.st;
    const PuzzleSrc<W> src{p.tab.info, p.tab.root, p.tab.open, p.tab.init, p.tab.row1};
    Env<W, TB> e;
    bool ok = false;
    if (in && rec) {
        const uint4* pc = rec + (size_t)g * R::kPieces;
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
                const uint32_t plen = (r[0] >> 16) & 0xFFu;
#pragma unroll
                for (int k = 0; k < kD; ++k) {
                    uint64_t d = r[R::kDirs + 2 * k] | ((uint64_t)r[R::kDirs + 2 * k + 1] << 32);
                    if constexpr (W == 1) d &= low_moves(plen - 1u, k);   // canonical, as k_restore stores it
                    s.dirs[k * kSnapBlock + t] = d;
                }
            }
            s.pos[t] = r[0];
            s.aux[t] = r[1];
            s.step[t] = r[2];
            s.pid[t] = r[3];
            e.load(q, src, t);
        }
    } else if (in) {
        const uint32_t pz = puzzle[g];
        ok = pz < p.tab.num_puzzles;
        if (ok) e.reset(q, src, pz);
    }
    if (in && !ok) atomicOr(p.err, (int)kErrSnapshot);
    const bool stop_done = rflags & kReplayStopDone, stop_illegal = rflags & kReplayStopIllegal;
    uint32_t n = 0;                                          // this sequence's actions
    if (ok) {
        n = len ? len[g] : L;
        n = n < L ? n : L;
    }
    const bool parked = ok && stop_done && e.pending;
    uint32_t end = !ok ? kRpInvalid : (parked ? kRpPending : kRpExhausted);
    bool live = ok && !parked && n > 0u;
    int code = 0, ret = 0;
    uint32_t f = 0, steps = 0, bad = ok ? 0xFFFFu : 0u;
    uint32_t a_next = (in && L > 0u) ? actions[g] : 0u;
    uint32_t ts = 0;
    for (; ts < L; ++ts) {
        if (__ballot(live) == 0ull) break;
        const uint32_t a = a_next;
        if (in && ts + 1u < L) a_next = actions[(size_t)(ts + 1u) * M + g];   // off this step's chain
        int sc = 0;
        uint32_t sf = 0;
        bool stepped = false;
        if (live) {
            if (stop_illegal && !(a < 4u && ((e.legal >> a) & 1u))) {
                end = kRpIllegal;
                bad = ts;
                live = false;
            } else {
                code = e.advance(q, src, a, f);
                ret += code;
                steps += 1u;
                sc = code;
                sf = f;
                stepped = true;
                if (stop_done && (f & 3u)) {
                    end = (f & 1u) ? kRpTerminated : kRpTruncated;
                    live = false;
                } else if (steps == n) {
                    live = false;
                }
            }
        }
        if (in) {
            const size_t at = (size_t)ts * M + g;
            if (o.step_code) o.step_code[at] = (int8_t)sc;
            if (o.step_flags) o.step_flags[at] = (uint8_t)sf;
            if constexpr (STATES) {
                uint32_t w[R::kWords];
#pragma unroll
                for (int k = 0; k < R::kWords; ++k) w[k] = 0;
                if (stepped) {
                    e.store(q, src, t);
                    replay_slot_words<W, TB>(s, t, w);
                }
                uint4* dst = o.states + at * R::kPieces;
#pragma unroll
                for (int k = 0; k < R::kPieces; ++k)
                    dst[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
            }
        }
    }
    if (in) {
        for (; ts < L; ++ts) {
            const size_t at = (size_t)ts * M + g;
            if (o.step_code) o.step_code[at] = 0;
            if (o.step_flags) o.step_flags[at] = 0;
            if constexpr (STATES) {
                uint4* dst = o.states + at * R::kPieces;
#pragma unroll
                for (int k = 0; k < R::kPieces; ++k) dst[k] = make_uint4(0u, 0u, 0u, 0u);
            }
        }
        if (o.code) o.code[g] = (int8_t)code;
        if (o.flags) o.flags[g] = (uint8_t)f;
        if (o.steps) o.steps[g] = (uint16_t)steps;
        if (o.end) o.end[g] = (uint8_t)end;
        if (o.ret) o.ret[g] = ret;
        if (o.bad) o.bad[g] = (uint16_t)bad;
    }
    if (!o.final_rec) return;   // the same for every thread of the grid
    uint32_t w[R::kWords];
#pragma unroll
    for (int k = 0; k < R::kWords; ++k) w[k] = 0;
    if (ok) {
        e.store(q, src, t);
        replay_slot_words<W, TB>(s, t, w);
    }
    __syncthreads();   // every slot has been read back: the LDS now takes the records
    uint4* wl = stage + wave * 64u * R::kPieces;
#pragma unroll
    for (int k = 0; k < R::kPieces; ++k)
        wl[lane * R::kPieces + k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    __syncthreads();
    // this wave's records are one contiguous run of the output: piece k*64 + lane per store
    const uint32_t g0 = blockIdx.x * kSnapBlock + wave * 64u;
    const uint32_t cnt = g0 < M ? (M - g0 < 64u ? M - g0 : 64u) : 0u;
    uint4* run = o.final_rec + (size_t)g0 * R::kPieces;
#pragma unroll
    for (int k = 0; k < R::kPieces; ++k) {
        const uint32_t qi = (uint32_t)k * 64u + lane;
        if (qi < cnt * R::kPieces) run[qi] = wl[qi];
    }
}

}  // namespace sparc
