// sparc_tables.hpp — the host's table builders: everything sparc_load_puzzles / sparc_load_rules
// derive from the caller's tables, as plain arrays.  Pure C++17 on std::vector: no HIP runtime
// call and no device code (only the vector types), so it runs on a CPU under sanitizers
// (tests/host/tables_main.cpp).  The loaders (sparc_kernels.hip) validate and build here, upload
// the arrays as they are, and commit.
#pragma once
#include <hip/hip_vector_types.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "sparc_gym_amd.h"
#include "sparc_layout.hpp"

namespace sparc {

// a builder's verdict: SPARC_OK, or the code and text the ABI call fails with
struct BuildError {
    int code = SPARC_OK;
    std::string msg;
    explicit operator bool() const { return code != SPARC_OK; }
};
inline BuildError invalid(const char* m) { return BuildError{SPARC_E_INVALID, m}; }

// where k_rolloutWs keeps a lane's board within a wave pair's LDS, and the LDS bytes it needs
// past the pairs: its own layout (sparc_kernels.hip kW_Board, splitw_fin_bytes)
struct SplitLds {
    uint32_t off_board;
    size_t fin_bytes;
};

// The device tables of one puzzle pool.  open and trie are uploaded from the caller's arrays.
struct HostPuzzleTables {
    uint32_t num_puzzles = 0, num_nodes = 0;
    std::vector<uint4> info;       // [P] device rows: w1 |= root terminal << 19, w3 = nodes | legal0 << 16
    std::vector<uint4> root;       // [P] trie record of each puzzle's root (sentinel if none)
    std::vector<uint64_t> init;    // [P] W = 1: free board at reset, one row up
    std::vector<uint4> row1;       // [P] W = 1: compact puzzle row
    // split-kernel tables (sparc_trie.hpp); empty when a puzzle's trie exceeds 15-bit nodes (!small)
    bool small = false;
    std::vector<uint2> trie8;      // 8-B records, each puzzle's on a 128-B line
    std::vector<uint2> trieg;      // [nodes][4]: the record of each node's field-d node
    std::vector<uint4> trow, mrow; // [P] trie rows, W = 1 move rows
    // W = 1 mixed tables (TrieLaneT<true>): 4-B records for tries of at most 127 nodes
    std::vector<uint8_t> trie4;
    std::vector<uint4> trow4;
    bool mixed_pays = false;       // the 8-B records outgrow an XCD's L2
    std::vector<uint32_t> nodes8;  // W = 1 and mixed_pays: trie nodes per puzzle (xcd_hot_bytes)
    // multi-word split kernel (k_rolloutWs); split_w false when the pool does not fit its layout
    bool split_w = false;
    SplitGeom sgeom{};
    std::vector<uint4> mroww;      // [P] move rows
    std::vector<uint32_t> boardw;  // [P][BS] reset boards
    bool ring_ok = false;          // W = 1 and every board fits below kRingShift
    uint64_t table_hash = 0;       // FNV-1a over the caller's arrays and the geometry
};

inline BuildError build_puzzle_tables(const sparc_puzzle_table* t, int W, uint32_t pitch, bool traceback,
                                      SplitLds lds, HostPuzzleTables& o) {
    if (!t || !t->open || !t->info) return invalid("null argument");
    if (t->num_puzzles < 1) return invalid("empty puzzle table");
    if (t->num_nodes < 0 || (t->num_nodes > 0 && !t->trie)) return invalid("bad trie");
    // validate every index the kernels will follow, so no launch can read out of bounds
    for (int q = 0; q < t->num_puzzles; ++q) {
        const uint32_t* inf = t->info + 4 * (size_t)q;
        const uint32_t X = inf[0] & 0xFF, Y = (inf[0] >> 8) & 0xFF;
        const uint32_t sx = (inf[0] >> 16) & 0xFF, sy = inf[0] >> 24;
        const uint32_t tx = inf[1] & 0xFF, ty = (inf[1] >> 8) & 0xFF, fl = inf[1] >> 16;
        const uint32_t base = inf[2], cnt = inf[3];
        char m[160];
        const bool fits = W == 1 ? (Y < pitch && pitch <= 15 && (X + 1) * pitch <= 64u)
                                 : (Y <= pitch && (X - 1) * pitch + Y <= 64u * W);
        if (X < 1 || Y < 1 || !fits) {
            snprintf(m, sizeof m, "puzzle %d: lattice %ux%u does not fit pitch %u / %d words%s", q, X, Y, pitch, W,
                     W == 1 ? " (words=1 needs the padded layout)" : "");
            return invalid(m);
        }
        if (sx >= X || sy >= Y || tx >= X || ty >= Y) {
            snprintf(m, sizeof m, "puzzle %d: start/target outside the lattice", q);
            return invalid(m);
        }
        // the path length is an 8-bit field of the state (pos bits 16-23, sparc_env.hpp) and of a
        // snapshot record: a path through every point a path can hold (the open points, and the
        // start even where it is closed) must stay at or below kMaxPathPoints
        uint32_t pts = 0;
        for (uint32_t x = 0; x < X; ++x)
            for (uint32_t y = 0; y < Y; ++y) {
                const uint32_t b = x * pitch + y;
                pts += (uint32_t)(((t->open[(size_t)q * W + (b >> 6)] >> (b & 63)) & 1ull) || (x == sx && y == sy));
            }
        if (pts > kMaxPathPoints) {
            snprintf(m, sizeof m, "puzzle %d: a path could hold %u points, at most %u fit (8-bit path length)", q, pts,
                     kMaxPathPoints);
            return invalid(m);
        }
        if ((fl & 2u) && (cnt == 0 || (uint64_t)base + cnt > (uint64_t)t->num_nodes || cnt > (W == 1 ? 0x7FFFu : 0xFFFFu))) {
            snprintf(m, sizeof m, "puzzle %d: trie range out of bounds", q);
            return invalid(m);
        }
        if (fl & 2u) {
            for (uint32_t k = 0; k < cnt; ++k) {
                const uint32_t* r = t->trie + 4 * ((size_t)base + k);
                const uint32_t ch[4] = {r[0] & 0xFFFF, r[0] >> 16, r[1] & 0xFFFF, r[1] >> 16};
                for (uint32_t v : ch)
                    if (v != kNone && v >= cnt) return invalid("trie child out of range");
                const uint32_t par = r[2] & 0xFFFF;
                if (k > 0 && par >= cnt) return invalid("trie parent out of range");
            }
        }
    }
    const size_t P = (size_t)t->num_puzzles;
    o = HostPuzzleTables{};
    o.num_puzzles = (uint32_t)t->num_puzzles;
    o.num_nodes = (uint32_t)t->num_nodes;
    auto rooted = [&](size_t q) { return ((t->info[4 * q + 1] >> 16) & 2u) != 0; };
    auto nodes = [&](size_t q) { return t->info[4 * q + 3] & 0xFFFFu; };
    // each puzzle's root record, so that a reset needs no dependent trie load
    o.root.assign(P, make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, kNone, 0u));
    for (size_t q = 0; q < P; ++q)
        if (rooted(q)) {
            const uint32_t* r = t->trie + 4 * (size_t)t->info[4 * q + 2];
            o.root[q] = make_uint4(r[0], r[1], r[2], r[3]);
        }
    // device copy of info: w3 = trie node count | legal mask of the reset state << 16, and for
    // the padded W = 1 layout the compact rows and the free board at reset
    o.info.resize(P);
    o.init.assign(P, 0);
    o.row1.assign(P, make_uint4(0u, 0u, 0u, 0u));
    for (size_t q = 0; q < P; ++q) {
        const uint32_t* inf = t->info + 4 * q;
        const uint32_t X = inf[0] & 0xFF, Y = (inf[0] >> 8) & 0xFF;
        const uint32_t sx = (inf[0] >> 16) & 0xFF, sy = inf[0] >> 24;
        auto open_at = [&](uint32_t x, uint32_t y) {
            const uint32_t b = x * pitch + y;
            return (t->open[q * W + (b >> 6)] >> (b & 63)) & 1ull;
        };
        uint32_t legal0 = 0;
        const int dx[4] = {1, 0, -1, 0}, dy[4] = {0, -1, 0, 1};
        for (int d = 0; d < 4; ++d) {
            const int nx = (int)sx + dx[d], ny = (int)sy + dy[d];
            if (nx >= 0 && ny >= 0 && nx < (int)X && ny < (int)Y && open_at(nx, ny)) legal0 |= 1u << d;
        }
        const uint32_t root_term = rooted(q) ? ((o.root[q].z >> 16) & 1u) : 0u;
        o.info[q] = make_uint4(inf[0], (inf[1] & 0x0007FFFFu) | (root_term << 19), inf[2],
                               (inf[3] & 0xFFFFu) | (legal0 << 16));
        if (W == 1) {
            const uint32_t tx = inf[1] & 0xFF, ty = (inf[1] >> 8) & 0xFF;
            // free board at reset, one row up (Env<1>): open points except the start
            o.init[q] = (t->open[q] & ~(1ull << (sx * pitch + sy))) << pitch;
            const uint32_t cnt = nodes(q);
            o.row1[q] = make_uint4((sx * pitch + sy) | ((tx * pitch + ty) << 8) | (o.info[q].y & 0xFFFF0000u),
                                   inf[2], (cnt ? cnt - 1u : 0u) | (legal0 << 16), 0u);
        }
    }
    // split-kernel tables (sparc_trie.hpp): 8-B records, field d = the child in direction d,
    // and the parent in the field of the direction back to it (the reverse of the move that
    // reached the node: no reachable child lives there, as that point is on the path); per
    // puzzle the trie row (root children, base, max node, flags) and, for W = 1, the move row
    o.small = true;
    for (size_t q = 0; q < P; ++q)
        if (rooted(q) && nodes(q) > 0x7FFFu) o.small = false;
    if (o.small) {
        // each puzzle's records start on a 128-B line (16 records; rootless puzzles: base 0): in
        // breadth-first order the root and the nodes near it, which most walks never leave,
        // share ONE line per puzzle instead of straddling two, so pools whose tries outgrow an
        // XCD's L2 refill fewer lines (the relative node indices, and so the env state, are
        // unchanged; only the split tables move)
        std::vector<size_t> b8(P, 0);
        size_t nn8 = 0;
        for (size_t q = 0; q < P; ++q) {
            if (!rooted(q)) continue;
            nn8 = (nn8 + 15u) & ~(size_t)15u;
            b8[q] = nn8;
            nn8 += nodes(q);
        }
        nn8 = std::max<size_t>(nn8, 1);
        if (W == 1)   // Env<1> (k_step, k_rollout1) reads trie8 at row1.y too
            for (size_t q = 0; q < P; ++q) o.row1[q].y = (uint32_t)b8[q];
        std::vector<uint2>& t8 = o.trie8;
        t8.assign(nn8, make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu));
        auto packed = [&](size_t base, uint32_t k) {   // node k of a puzzle as index | terminal << 15
            return k | (((t->trie[4 * (base + k) + 2] >> 16) & 1u) << 15);
        };
        for (size_t q = 0; q < P; ++q) {
            if (!rooted(q)) continue;
            const size_t base = t->info[4 * q + 2], bq = b8[q];
            const uint32_t cnt = nodes(q);
            for (uint32_t k = 0; k < cnt; ++k) {
                const uint32_t* r = t->trie + 4 * (base + k);
                const uint32_t ch[4] = {r[0] & 0xFFFFu, r[0] >> 16, r[1] & 0xFFFFu, r[1] >> 16};
                uint32_t f[4];
                for (int d = 0; d < 4; ++d) f[d] = ch[d] == kNone ? 0xFFFFu : packed(base, ch[d]);
                t8[bq + k] = make_uint2(f[0] | (f[1] << 16), f[2] | (f[3] << 16));
            }
            for (uint32_t k = 0; k < cnt; ++k) {           // parents, after every child field
                const uint32_t* r = t->trie + 4 * (base + k);
                const uint32_t ch[4] = {r[0] & 0xFFFFu, r[0] >> 16, r[1] & 0xFFFFu, r[1] >> 16};
                for (uint32_t d = 0; d < 4; ++d) {
                    if (ch[d] == kNone) continue;
                    uint2& cr = t8[bq + ch[d]];
                    const uint32_t back = d ^ 2u, sh = (back & 1u) * 16u;
                    uint32_t& w = back < 2 ? cr.x : cr.y;
                    w = (w & ~(0xFFFFu << sh)) | (packed(base, k) << sh);
                }
            }
        }
        o.trow.resize(P);
        o.mrow.assign(P, make_uint4(0u, 0u, 0u, 0u));
        for (size_t q = 0; q < P; ++q) {
            const uint32_t fl = (o.info[q].y >> 16) & 0xFFFFu;
            const uint32_t cnt = nodes(q);
            const uint2 rr = (fl & 2u) ? t8[b8[q]] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
            // flags as row1: bit0 solutions, bit1 root valid, bit3 root terminal
            const uint32_t tf = (fl & 3u) | (((o.info[q].y >> 19) & 1u) << 3);
            const uint32_t rootS = (tf & 2u) ? ((tf >> 3) & 1u) << 15 : 0x10000u;
            o.trow[q] = make_uint4(rr.x, rr.y, (uint32_t)b8[q], rootS | ((tf & 1u) << 14) | ((cnt ? cnt - 1u : 0u) << 17));
            // W = 1 move row: row word, reset board, and the puzzle the autoreset after it loads
            if (W == 1) o.mrow[q] = make_uint4(o.row1[q].x, (uint32_t)o.init[q], (uint32_t)(o.init[q] >> 32),
                                               q + 1 == P ? 0u : (uint32_t)q + 1u);
        }
        // look-ahead records (TrieLane::step1la): entry 4k + d = the record of node k's field-d
        // node (child, or the parent in the back direction), all ones where the field is empty;
        // at least 4 entries, so that a rootless puzzle's lane (base 0, node 0) reads in bounds
        o.trieg.assign(4 * nn8, make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu));
        for (size_t q = 0; q < P; ++q) {
            if (!rooted(q)) continue;
            const size_t base = b8[q];
            const uint32_t cnt = nodes(q);
            for (uint32_t k = 0; k < cnt; ++k) {
                const uint2 r = t8[base + k];
                const uint32_t f[4] = {r.x & 0xFFFFu, r.x >> 16, r.y & 0xFFFFu, r.y >> 16};
                for (int d = 0; d < 4; ++d)
                    if (f[d] != 0xFFFFu) o.trieg[4 * (base + k) + d] = t8[base + (f[d] & 0x7FFFu)];
            }
        }
        // mixed tables (TrieLaneT<true>): a trie of at most 127 nodes as 4-B records (each 16-bit
        // field of trie8 as an 8-bit one, index | terminal << 7, 0xFF none), a larger one as its
        // 8-B records; each puzzle's records start on a 128-B line, the base is a byte offset, and
        // bit 13 of the row's w marks a compact puzzle (root S then 0x80 / 0x100).  Used when the
        // 8-B records outgrow an XCD's 4 MB L2: below that the per-lane format costs the trie chain
        // more than the misses it saves (MI355X, c3: 4,096 puzzles, 2 MB of records, +5 %; 16,384
        // puzzles, 8.4 MB, -7.4 %; profiles/r06/ab_bigpool); SPARC_VARIANT_MIXED_TRIE overrides
        o.mixed_pays = nn8 * sizeof(uint2) > kMixedTrieBytes;
        if (W == 1 && o.mixed_pays) {   // sparc_reset_host refines the choice per XCD (xcd_hot_bytes)
            o.nodes8.resize(P);
            for (size_t q = 0; q < P; ++q) o.nodes8[q] = nodes(q);
        }
        if (W == 1) {
            std::vector<size_t> bo(P, 0);
            size_t nb = 0;
            auto tiny = [&](size_t q) { return nodes(q) <= 127u; };
            for (size_t q = 0; q < P; ++q) {
                if (!rooted(q)) continue;
                nb = (nb + 127u) & ~(size_t)127u;
                bo[q] = nb;
                nb += (size_t)nodes(q) * (tiny(q) ? 4u : 8u);
            }
            nb += 8;   // an 8-B gather of the last 4-B record stays in bounds
            auto f8 = [](uint32_t f16) { return f16 == 0xFFFFu ? 0xFFu : (f16 & 0x7Fu) | ((f16 >> 15) << 7); };
            auto rec4 = [&](uint2 r) {
                return f8(r.x & 0xFFFFu) | (f8(r.x >> 16) << 8) | (f8(r.y & 0xFFFFu) << 16) | (f8(r.y >> 16) << 24);
            };
            o.trie4.assign(nb, 0xFF);
            o.trow4.resize(P);
            for (size_t q = 0; q < P; ++q) {
                const uint32_t cnt = nodes(q);
                const bool small4 = rooted(q) && tiny(q);
                const uint32_t w = o.trow[q].w;
                uint2 root = make_uint2(o.trow[q].x, o.trow[q].y);
                if (rooted(q)) {
                    for (uint32_t k = 0; k < cnt; ++k) {
                        const uint2 r8 = t8[b8[q] + k];
                        if (small4) {
                            const uint32_t v = rec4(r8);
                            memcpy(&o.trie4[bo[q] + 4 * (size_t)k], &v, 4);
                        } else {
                            memcpy(&o.trie4[bo[q] + 8 * (size_t)k], &r8, 8);
                        }
                    }
                    if (small4) root = make_uint2(rec4(root), 0xFFFFFFFFu);
                }
                // root S 0x80 (terminal) / 0x100 (off the trie) in the compact layout
                const uint32_t rs = small4 ? ((w & 0x10000u) ? 0x100u : ((w >> 15) & 1u) << 7) : (w & 0x18000u);
                o.trow4[q] = make_uint4(root.x, root.y, (uint32_t)bo[q],
                                        rs | (small4 ? 1u << 13 : 0u) | (w & 0x4000u) | (w & ~0x1FFFFu));
            }
        }
        // multi-word split geometry (sparc_movew.hpp): internal pitch + 1, the board plus a
        // zero row above and one spare dword, the longest possible path in the move stack
        if (W > 1 && pitch <= 15u) {
            SplitGeom g{};
            g.P2 = pitch + 1u;
            uint32_t xmax = 1, pts = 1;
            for (size_t q = 0; q < P; ++q) {
                const uint32_t X = t->info[4 * q] & 0xFFu, Y = (t->info[4 * q] >> 8) & 0xFFu;
                xmax = std::max(xmax, X);
                pts = std::max(pts, X * Y);
            }
            g.B = ((xmax + 2u) * g.P2 + 31u) / 32u + 1u;
            g.BS = (g.B + 3u) & ~3u;
            // the move wave writes slot len - 1 on every step, moved or not, and len reaches pts
            // on a path through every point: pts slots, not pts - 1
            g.M = traceback ? ((pts + 15u) & ~15u) : 0u;
            g.nbr_pos = (2u * g.P2) | ((g.P2 - 1u) << 8) | (0u << 16) | ((g.P2 + 1u) << 24);
            g.off_board = lds.off_board;
            g.off_stack = g.off_board + g.BS * 256u;
            g.pair = (g.off_stack + g.M * 64u + 15u) & ~15u;
            // the move wave keeps the next reset board in kBoardRegs 16-B registers
            if (4 * (size_t)g.pair + lds.fin_bytes <= kMaxDynLds && g.BS <= 4u * kBoardRegs) {
                o.mroww.resize(P);
                o.boardw.assign(P * g.BS, 0u);
                for (size_t q = 0; q < P; ++q) {
                    const uint32_t* inf = t->info + 4 * q;
                    const uint32_t X = inf[0] & 0xFF, Y = (inf[0] >> 8) & 0xFF;
                    const uint32_t sx = (inf[0] >> 16) & 0xFF, sy = inf[0] >> 24;
                    const uint32_t tx = inf[1] & 0xFF, ty = (inf[1] >> 8) & 0xFF;
                    o.mroww[q] = make_uint4((sx * g.P2 + sy) | ((tx * g.P2 + ty) << 16), (inf[1] >> 16) & 7u, 0u, 0u);
                    for (uint32_t x = 0; x < X; ++x)
                        for (uint32_t y = 0; y < Y; ++y) {
                            const uint32_t b = x * pitch + y;
                            if (!((t->open[q * W + (b >> 6)] >> (b & 63)) & 1ull) || (x == sx && y == sy)) continue;
                            const uint32_t d = (x + 1u) * g.P2 + y;
                            o.boardw[q * g.BS + (d >> 5)] |= 1u << (d & 31u);
                        }
                }
                o.sgeom = g;
                o.split_w = true;
            }
        }
    }
    o.ring_ok = W == 1;
    for (size_t q = 0; q < P; ++q)
        if ((t->info[4 * q] & 0xFFu) * pitch > kRingShift) o.ring_ok = false;
    // identity of the table for snapshots (sparc_snapshot_info): FNV-1a over the host arrays
    uint64_t h = 0xCBF29CE484222325ull;
    auto mix = [&h](const void* d, size_t bytes) {
        const uint8_t* b = static_cast<const uint8_t*>(d);
        for (size_t k = 0; k < bytes; ++k) h = (h ^ b[k]) * 0x100000001B3ull;
    };
    const int32_t head[4] = {t->num_puzzles, t->num_nodes, (int32_t)pitch, W};
    mix(head, sizeof head);
    mix(t->open, sizeof(uint64_t) * P * W);
    mix(t->info, sizeof(uint32_t) * 4 * P);
    if (t->num_nodes > 0) mix(t->trie, sizeof(uint32_t) * 4 * (size_t)t->num_nodes);
    o.table_hash = h;
    return BuildError{};
}

// The 8-B trie records one XCD's L2 must hold for the envs of a full reset: k_rollout1s runs 256
// envs per workgroup and workgroups b, b + 8, ... share an XCD (round-robin dispatch,
// MI355X_MICROARCH.md), so XCD group g holds envs i with (i / 256) % 8 == g, and each env plays
// its start puzzle and the next kHotWalk - 1.  Returns the largest group's bytes.  A pool whose
// envs are placed XCD-locally (bench.initial_puzzles 'xcd') keeps the 8-B records past 4 MB of
// them (MI355X, c3 at 16,384 puzzles: 0.362 ms with 8-B records against 0.379 ms mixed; the
// hash placement 0.405 ms, mixed 0.394; profiles/r06/ab_xcd_place).
inline size_t xcd_hot_bytes(const std::vector<uint32_t>& nodes8, const uint32_t* q, uint32_t n) {
    const uint32_t P = (uint32_t)nodes8.size();
    std::vector<uint8_t> seen(P, 0);   // bit g: counted for group g
    size_t bytes[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t g = (i / 256u) & 7u;
        uint32_t u = q[i];
        for (uint32_t k = 0; k < kHotWalk; ++k, u = u + 1 == P ? 0u : u + 1) {
            if (seen[u] & (1u << g)) continue;
            seen[u] |= (uint8_t)(1u << g);
            bytes[g] += (size_t)nodes8[u] * sizeof(uint2);
        }
    }
    return *std::max_element(bytes, bytes + 8);
}

// The device tables of one rule table, and the host copies for the exact fits the host finishes
// (searches past the node cap, kHostFit puzzles).  inst, shape_area and shape_off are the caller's
// arrays, padded to one entry when empty.
struct HostRuleTables {
    std::vector<uint2> shape_range;   // [S] {first offset, count}
    std::vector<uint2> inst_fc;       // [P] {first, count | kHostFit}
    std::vector<uint32_t> inst;
    std::vector<int32_t> shape_area;
    std::vector<int8_t> shape_off;
    std::vector<uint64_t> planes;     // [P][RP_COUNT][W]
    bool area_ok = true;              // every cell's net area fits the kAreaPlanes planes
    size_t host_fit_puzzles = 0;      // puzzles flagged kHostFit
    // region-code table (sparc_rules.hpp): each puzzle's first entry or kNoRegTab, the table's
    // words, and the (puzzle, word) work list of k_region_table
    std::vector<uint32_t> reg_off;
    std::vector<uint2> items;
    size_t reg_words = 0;
    bool tab_all = false;             // every puzzle has a region-code table
};

// info: the loaded puzzle table's device rows (HostPuzzleTables::info); reg_entries: the
// region-code table's budget in 4-bit entries
inline BuildError build_rule_tables(const sparc_rules_table* t, const std::vector<uint4>& info, int W,
                                    size_t reg_entries, HostRuleTables& o) {
    if (!t || !t->planes || !t->inst_first || !t->shape_first) return invalid("null argument");
    if ((size_t)(uint32_t)t->num_puzzles != info.size())
        return invalid("rule table puzzle count differs from the loaded puzzle table");
    if (t->num_inst < 0 || t->num_shapes < 0 || t->num_offsets < 0 || t->num_shapes >= (1 << 21) ||
        (t->num_inst && !t->inst) || (t->num_shapes && !t->shape_area) || (t->num_offsets && !t->shape_off))
        return invalid("bad rule table sizes");
    const size_t P = info.size(), S = (size_t)t->num_shapes;
    o = HostRuleTables{};
    // the device's ranges: {first, count} per shape and {first, count | kHostFit} per puzzle
    o.shape_range.assign(std::max<size_t>(1, S), make_uint2(0u, 0u));
    o.inst_fc.resize(P);
    if (t->shape_first[0] != 0) return invalid("shape offsets must start at 0");
    for (size_t sh = 0; sh < S; ++sh) {
        const uint32_t o0 = t->shape_first[sh], o1 = t->shape_first[sh + 1];
        if (o1 < o0 || o1 > (uint32_t)t->num_offsets) return invalid("shape offsets out of range");
        o.shape_range[sh] = make_uint2(o0, o1 - o0);
    }
    if (t->inst_first[0] != 0) return invalid("instance offsets must start at 0");
    for (size_t q = 0; q < P; ++q) {
        const uint32_t X = info[q].x & 0xFFu, Y = (info[q].x >> 8) & 0xFFu;
        const uint32_t f = t->inst_first[q], f1 = t->inst_first[q + 1];
        char m[160];
        if (X > 15 || Y > 15) {
            snprintf(m, sizeof m, "puzzle %zu: the rule audit supports lattices up to 15x15", q);
            return invalid(m);
        }
        if (f1 < f || f1 > (uint32_t)t->num_inst) return invalid("instance range out of bounds");
        const uint32_t n = f1 - f;
        const uint32_t cells = ((X - 1) / 2) * ((Y - 1) / 2);
        if (n > cells) {   // _extract_poly_instances: one instance per cell centre
            snprintf(m, sizeof m, "puzzle %zu: %u instances on %u cells", q, n, cells);
            return invalid(m);
        }
        int ny = 0, nd = 0;
        uint32_t ds[kHostFitMax];
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t e = t->inst[f + k], b = e & 0x3FFu, sh = e >> 11;
            if (b >= 64u * W || sh >= (uint32_t)S) return invalid("bad instance");
            if ((e >> 10) & 1u) { ++ny; continue; }
            int j = 0;
            while (j < nd && ds[j] != sh) ++j;
            if (j == nd) ds[nd++] = sh;
        }
        // past the GPU search's list sizes: the puzzle's searches run on the host (kHostFit)
        const bool hf = ny > kFitYlops || nd > kFitShapes;
        o.host_fit_puzzles += hf;
        o.inst_fc[q] = make_uint2(f, n | (hf ? kHostFit : 0u));
    }
    // the device copy: the caller's SPARC_RULE_PLANES planes per puzzle, RP_INST rewritten from the
    // instance list, then the bit-sliced net area of each cell (kAreaPlanes planes, sparc_rules.hpp)
    static_assert(RP_ABI == SPARC_RULE_PLANES, "rule plane layout");
    o.planes.assign(P * RP_COUNT * W, 0ull);
    for (size_t q = 0; q < P; ++q) {
        uint64_t* d = o.planes.data() + q * RP_COUNT * W;
        std::copy(t->planes + q * RP_ABI * W, t->planes + (q + 1) * RP_ABI * W, d);
        for (int k = 0; k < W; ++k) d[RP_INST * W + k] = 0;
        int32_t net[256] = {0};
        const uint32_t f = o.inst_fc[q].x, n = o.inst_fc[q].y & ~kHostFit;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t e = t->inst[f + k], b = e & 0x3FFu;
            const int64_t a = t->shape_area[e >> 11];
            net[b] = (int32_t)std::max<int64_t>(-(1 << 20), std::min<int64_t>(1 << 20, net[b] + (((e >> 10) & 1u) ? -a : a)));
            d[RP_INST * W + (b >> 6)] |= 1ull << (b & 63);
        }
        // a cell's net area outside -128..127: the audit walks the list instead
        for (uint32_t b = 0; b < 64u * W; ++b) {
            if (net[b] < -(1 << (kAreaPlanes - 1)) || net[b] >= (1 << (kAreaPlanes - 1))) o.area_ok = false;
            for (int k = 0; k < kAreaPlanes; ++k)
                if (((uint32_t)net[b] >> k) & 1u) d[(RP_AREA0 + k) * W + (b >> 6)] |= 1ull << (b & 63);
        }
    }
    o.inst.assign(t->inst, t->inst + t->num_inst);
    o.inst.resize(std::max<size_t>(1, t->num_inst), 0u);
    o.shape_area.assign(t->shape_area, t->shape_area + S);
    o.shape_area.resize(std::max<size_t>(1, S), 0);
    o.shape_off.assign(t->shape_off, t->shape_off + 2 * (size_t)t->num_offsets);
    o.shape_off.resize(2 * std::max<size_t>(1, t->num_offsets), 0);
    // the per-region check code (squares, stars, poly/ylop area + exact fit) of every region cell
    // mask of each puzzle with at most kRegTabCells cells, computed once at the load by the audit's
    // own region_code (k_region_table): the audit then looks codes up per region instead of running
    // the checks (the memo serves the larger puzzles, and the puzzles past the table budget:
    // 2^28 entries, 128 MB, unless sparc_set_rule_limits sets another)
    o.reg_off.assign(P, kNoRegTab);
    size_t entries = 0;
    for (size_t q = 0; q < P; ++q) {
        const uint32_t X = info[q].x & 0xFFu, Y = (info[q].x >> 8) & 0xFFu;
        const uint32_t cells = ((X - 1) / 2) * ((Y - 1) / 2);
        if (cells > kRegTabCells) continue;
        const uint32_t words = cells <= 3 ? 1u : 1u << (cells - 3);
        if (entries + 8u * words > reg_entries) break;
        o.reg_off[q] = (uint32_t)entries;
        for (uint32_t g = 0; g < words; ++g) o.items.push_back(make_uint2((uint32_t)q, g));
        entries += 8u * words;
    }
    o.reg_words = entries / 8;
    o.tab_all = std::none_of(o.reg_off.begin(), o.reg_off.end(), [](uint32_t v) { return v == kNoRegTab; });
    return BuildError{};
}

// the audit's per-puzzle rows (RulesTab::rows): base planes, table offset, instance range, info
inline std::vector<uint64_t> build_rule_rows(const HostRuleTables& r, const std::vector<uint4>& info, int W) {
    const size_t P = info.size();
    const size_t RW = W == 1 ? rule_row_u64<1>() : W == 2 ? rule_row_u64<2>() : rule_row_u64<4>();
    std::vector<uint64_t> rows(P * RW, 0ull);
    for (size_t q = 0; q < P; ++q) {
        uint64_t* row = rows.data() + q * RW;
        for (int k = 0; k < 10; ++k)
            for (int w = 0; w < W; ++w) row[k * W + w] = r.planes[(q * RP_COUNT + kBasePlanes[k]) * W + w];
        // info.y bits 24-31 (free: flags use 16-18) carry the instance count | kHostFit << 7
        const uint2 fc = r.inst_fc[q];
        const uint32_t cf = (fc.y & 0x7Fu) | ((fc.y & kHostFit) ? 0x80u : 0u);
        row[10 * W] = (uint64_t)r.reg_off[q] | ((uint64_t)fc.x << 32);
        row[10 * W + 1] = (uint64_t)info[q].x | ((uint64_t)((info[q].y & 0x00FFFFFFu) | (cf << 24)) << 32);
    }
    return rows;
}

// ---- the host mirror of HostFits (sparc_rules.hpp): answers of the host's exact fits
// one answer into the table (false: already there); the load factor stays <= 1/2
inline bool hostfits_insert(std::vector<uint4>& t, uint32_t q, uint64_t rm, uint32_t fits) {
    const uint32_t mask = (uint32_t)t.size() - 1u;
    for (uint32_t s = hostfit_slot(q, rm, mask);; s = (s + 1u) & mask) {
        uint4& e = t[s];
        if (!(e.w & 2u)) {
            e = make_uint4((uint32_t)rm, (uint32_t)(rm >> 32), q, fits | 2u);
            return true;
        }
        if (e.x == (uint32_t)rm && e.y == (uint32_t)(rm >> 32) && e.z == q) return false;
    }
}
// The table grows to keep its load factor <= 1/2 with `need` answers, up to kHostFitsMax slots
// (64 MB); past that new answers are not kept (audits then queue those searches again; the
// results are the same).  True: the table was rebuilt at a larger size.
constexpr size_t kHostFitsMin = (size_t)1 << 12, kHostFitsMax = (size_t)1 << 22;
inline bool hostfits_grow(std::vector<uint4>& tab, size_t need) {
    const size_t cap = tab.size();
    if (2 * need <= cap || cap >= kHostFitsMax) return false;
    size_t ncap = std::max(cap, kHostFitsMin);
    while (2 * need > ncap && ncap < kHostFitsMax) ncap *= 2;
    std::vector<uint4> t(ncap, make_uint4(0u, 0u, 0u, 0u));
    for (const uint4& e : tab)
        if (e.w & 2u) hostfits_insert(t, e.z, (uint64_t)e.x | ((uint64_t)e.y << 32), e.w & 1u);
    tab.swap(t);
    return true;
}

}  // namespace sparc
