// sparc_layout.hpp — table formats and limits that the host's table builders (sparc_tables.hpp)
// and the kernels share.  No device code and no HIP include: this header also compiles as plain
// C++ (the host builders run on a CPU under sanitizers, tests/host/tables_main.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__)
#define SPARC_HD __attribute__((host)) __attribute__((device))
#else
#define SPARC_HD
#endif

namespace sparc {

constexpr uint32_t kNone = 0xFFFFu;         // no child in a trie record's 16-bit field
constexpr size_t kMaxDynLds = 160 * 1024;   // one workgroup may own all 160 KiB (gfx950)
// points of the longest path: the length is 8 bits of the state's pos word and of a snapshot
// record (bits 16-23), so the loaders refuse a puzzle whose path could hold more
constexpr uint32_t kMaxPathPoints = 255;

// W = 1 split kernel (k_rollout1s): the pitches its window arithmetic covers
SPARC_HD constexpr bool split1_pitch_ok(uint32_t P) { return P >= 3u && P <= 9u; }

// runtime layout of k_rolloutWs, computed by the host for the pool (build_puzzle_tables)
struct SplitGeom {
    uint32_t P2;        // internal pitch (<= 16: the window's right neighbour is bit 2 * P2 <= 32)
    uint32_t B;         // board dwords per lane (board + one zero dword above the top row)
    uint32_t BS;        // B rounded up to 4: dwords per lane in LDS and per puzzle in the reset-board table
    uint32_t M;         // move-stack bytes per lane (>= the lattice's point count, multiple of 16:
                        // a step writes slot len - 1 even when it does not move, and len <= points)
    uint32_t nbr_pos;   // window bit of each direction's neighbour, one byte per direction
    uint32_t pair;      // LDS bytes per move / trie wave pair
    uint32_t off_board, off_stack;   // their offsets within a pair
};
constexpr uint32_t kBoardRegs = 4;   // 16-B pieces of the next reset board kept in registers

// k_rollout1r's ring word: the board in the bits below kRingShift (every W = 1 pool with
// x_size * pitch <= 57)
constexpr uint32_t kRingShift = 57;

constexpr size_t kMixedTrieBytes = (size_t)4 << 20;   // an XCD's L2: past it the mixed trie tables pay
// puzzles an env plays per 2,000-step launch under random actions (episodes of ~300 steps, next
// puzzle on each autoreset): the window of its start puzzle that xcd_hot_bytes counts
constexpr uint32_t kHotWalk = 8;

// rule-plane indices of include/sparc_gym_amd.h (SPARC_RULE_PLANES), then the planes the loader
// (build_rule_tables) derives from the instance list for the device copy: the net instance area
// of each cell (Σ poly areas − Σ ylop areas of the instances there, 8-bit two's complement,
// bit-sliced), so a region's area check (_polyfit_check_area 700-709) is 8 popcounts instead of
// a walk over the puzzle's instance list with two dependent loads per instance.  RP_INST of the
// device copy is rewritten from the list too (cells holding an instance).
enum : uint32_t {
    RP_CELLS = 0, RP_LATTICE, RP_GAPS, RP_DOTS, RP_TRI, RP_TRI0, RP_TRI1, RP_TRI2, RP_STAR, RP_SQUARE,
    RP_COLORED, RP_COL1, RP_M0 = RP_COL1 + 8, RP_M1, RP_M2, RP_NOTFIRST, RP_NOTLAST, RP_INST, RP_ABI,
    RP_AREA0 = RP_ABI, RP_COUNT = RP_AREA0 + 8
};
constexpr int kAreaPlanes = 8;
// The GPU's search keeps its per-region lists in registers / scratch of these sizes; a puzzle with
// more ylops or distinct poly shapes (instances sit at cell centres, one per cell, so never more
// than 64 of either) is flagged by the loader (kHostFit) and its searches run on the host
// (exact_fit<..., kHostFitMax, kHostFitMax, kHostFitPlanes>, sparc_kernels.hip host_fit)
constexpr int kFitYlops = 16;
constexpr int kFitShapes = 16;
constexpr int kHostFitMax = 64, kHostFitPlanes = 8;   // every valid puzzle: <= 64 cells, counts >= -65
constexpr uint32_t kHostFit = 0x80000000u;            // instance count flag: searches on the host

// slot of (puzzle, region cells) in the HostFits table (sparc_rules.hpp); mask = slots - 1
SPARC_HD inline __attribute__((always_inline)) uint32_t hostfit_slot(uint32_t q, uint64_t rm, uint32_t mask) {
    uint64_t h = rm * 0x9E3779B97F4A7C15ull ^ ((uint64_t)q * 0xC2B2AE3D27D4EB4Full);
    h ^= h >> 29;
    return (uint32_t)h & mask;
}

// the audit's per-puzzle row (RulesTab::rows): the kBasePlanes planes, then two words
template <int W>
SPARC_HD constexpr uint32_t rule_row_u64() { return 10u * W + 2u; }
constexpr uint32_t kBasePlanes[10] = {RP_CELLS, RP_LATTICE, RP_GAPS, RP_DOTS, RP_TRI, RP_TRI0, RP_TRI1, RP_TRI2,
                                      RP_NOTFIRST, RP_NOTLAST};
constexpr uint32_t kNoRegTab = 0xFFFFFFFFu;   // reg_off of a puzzle without a region-code table
constexpr uint32_t kRegTabCells = 12;         // cells of the largest puzzle that gets one

}  // namespace sparc
