// tables_main.cpp — the host table builders (sparc_tables.hpp) on a CPU, for sanitizer builds.
//
//   tables_main check  DIR...   build each pool's tables and compare them with expectations that
//                               are derived here from the input tables alone
//   tables_main reject DIR...   print "<code>|<text>" of each table's rejection
//   tables_main hostfits        the HostFits mirror and xcd_hot_bytes
//
// DIR holds meta.txt (key value lines) and the raw arrays of tests/test_tables_host.py; a missing
// array file is a null pointer.  Includes only the two host-side headers.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "sparc_layout.hpp"
#include "sparc_tables.hpp"

using namespace sparc;

namespace {

int g_fail = 0;
std::string g_where;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++g_fail <= 40) {                          \
                printf("FAIL %s: %s | ", g_where.c_str(), #cond); \
                printf(__VA_ARGS__);                       \
                printf("\n");                              \
            }                                              \
        }                                                  \
    } while (0)

// k_rolloutWs's LDS layout as the library passes it today (the builder takes it as given)
const SplitLds kLds{14336u, 8192u};

template <class T>
struct Arr {
    std::vector<T> v;
    bool present = false;
    // exactly the file's elements, so that a read past the end is a sanitizer report; an empty
    // array that is present is still a non-null pointer
    const T* ptr() const {
        static const T none{};
        return !present ? nullptr : v.empty() ? &none : v.data();
    }
};
template <class T>
Arr<T> read_arr(const std::string& dir, const char* name) {
    Arr<T> a;
    std::ifstream f(dir + "/" + name, std::ios::binary);
    if (!f) return a;
    a.present = true;
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    a.v.resize(raw.size() / sizeof(T));
    if (!raw.empty()) memcpy(a.v.data(), raw.data(), raw.size());
    return a;
}

struct Pool {
    std::map<std::string, long long> meta;
    Arr<uint64_t> open, planes;
    Arr<uint32_t> info, trie, inst_first, inst, shape_first;
    Arr<int32_t> shape_area;
    Arr<int8_t> shape_off;
    sparc_puzzle_table pt{};
    sparc_rules_table rt{};
    int W = 1;
    uint32_t pitch = 0;
    bool tb = false;
    long long get(const char* k, long long dflt) const {
        auto it = meta.find(k);
        return it == meta.end() ? dflt : it->second;
    }
};

Pool load_pool(const std::string& dir) {
    Pool p;
    std::ifstream m(dir + "/meta.txt");
    std::string k;
    long long v;
    while (m >> k >> v) p.meta[k] = v;
    p.open = read_arr<uint64_t>(dir, "open.bin");
    p.info = read_arr<uint32_t>(dir, "info.bin");
    p.trie = read_arr<uint32_t>(dir, "trie.bin");
    p.planes = read_arr<uint64_t>(dir, "planes.bin");
    p.inst_first = read_arr<uint32_t>(dir, "inst_first.bin");
    p.inst = read_arr<uint32_t>(dir, "inst.bin");
    p.shape_first = read_arr<uint32_t>(dir, "shape_first.bin");
    p.shape_area = read_arr<int32_t>(dir, "shape_area.bin");
    p.shape_off = read_arr<int8_t>(dir, "shape_off.bin");
    p.W = (int)p.get("words", 1);
    p.pitch = (uint32_t)p.get("pitch", 0);
    p.tb = p.get("traceback", 0) != 0;
    p.pt = sparc_puzzle_table{(int32_t)p.get("num_puzzles", 0), (int32_t)p.get("num_nodes", 0), p.open.ptr(),
                              p.info.ptr(), p.trie.ptr()};
    p.rt = sparc_rules_table{(int32_t)p.get("rule_puzzles", p.get("num_puzzles", 0)), (int32_t)p.get("num_inst", 0),
                             (int32_t)p.get("num_shapes", 0), (int32_t)p.get("num_offsets", 0), p.planes.ptr(),
                             p.inst_first.ptr(), p.inst.ptr(), p.shape_first.ptr(), p.shape_area.ptr(), p.shape_off.ptr()};
    return p;
}

bool eq(uint4 a, uint4 b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }
bool eq(uint2 a, uint2 b) { return a.x == b.x && a.y == b.y; }
bool ones(uint2 a) { return a.x == 0xFFFFFFFFu && a.y == 0xFFFFFFFFu; }
uint32_t field(uint2 r, uint32_t d) { return ((d < 2 ? r.x : r.y) >> (16u * (d & 1u))) & 0xFFFFu; }

// the input table, read per puzzle
struct Src {
    const Pool& p;
    uint32_t X(size_t q) const { return p.info.v[4 * q] & 0xFFu; }
    uint32_t Y(size_t q) const { return (p.info.v[4 * q] >> 8) & 0xFFu; }
    uint32_t sx(size_t q) const { return (p.info.v[4 * q] >> 16) & 0xFFu; }
    uint32_t sy(size_t q) const { return p.info.v[4 * q] >> 24; }
    uint32_t tx(size_t q) const { return p.info.v[4 * q + 1] & 0xFFu; }
    uint32_t ty(size_t q) const { return (p.info.v[4 * q + 1] >> 8) & 0xFFu; }
    uint32_t flags(size_t q) const { return p.info.v[4 * q + 1] >> 16; }
    bool rooted(size_t q) const { return (flags(q) & 2u) != 0; }
    size_t base(size_t q) const { return p.info.v[4 * q + 2]; }
    uint32_t cnt(size_t q) const { return p.info.v[4 * q + 3] & 0xFFFFu; }
    const uint32_t* node(size_t q, uint32_t k) const { return &p.trie.v[4 * (base(q) + k)]; }
    uint32_t child(size_t q, uint32_t k, uint32_t d) const { return (node(q, k)[d >> 1] >> (16u * (d & 1u))) & 0xFFFFu; }
    uint32_t parent(size_t q, uint32_t k) const { return node(q, k)[2] & 0xFFFFu; }
    uint32_t term(size_t q, uint32_t k) const { return (node(q, k)[2] >> 16) & 1u; }
    bool open_at(size_t q, uint32_t x, uint32_t y) const {
        const uint32_t b = x * p.pitch + y;
        return (p.open.v[q * p.W + (b >> 6)] >> (b & 63u)) & 1ull;
    }
};

void check_puzzles(const Pool& p, const HostPuzzleTables& h) {
    const Src s{p};
    const size_t P = (size_t)p.pt.num_puzzles;
    const int W = p.W;
    const uint32_t pitch = p.pitch;
    CHECK(h.num_puzzles == P && h.num_nodes == (uint32_t)p.pt.num_nodes, "counts");
    CHECK(h.info.size() == P && h.root.size() == P && h.init.size() == P && h.row1.size() == P, "row counts");
    bool small = true;
    for (size_t q = 0; q < P; ++q)
        if (s.rooted(q) && s.cnt(q) > 0x7FFFu) small = false;
    CHECK(h.small == small, "small %d", (int)h.small);
    CHECK(small == (bool)p.get("expect_small", 1), "the pool reaches the branch the test means");
    // bases: 16-record lines for trie8, 128-B lines for trie4
    std::vector<size_t> b8(P, 0), b4(P, 0);
    size_t end8 = 0, end4 = 0;
    for (size_t q = 0; q < P; ++q) {
        if (!s.rooted(q)) continue;
        b8[q] = (end8 + 15) / 16 * 16;
        end8 = b8[q] + s.cnt(q);
        b4[q] = (end4 + 127) / 128 * 128;
        end4 = b4[q] + (size_t)s.cnt(q) * (s.cnt(q) <= 127 ? 4 : 8);
    }
    uint32_t n_rootless = 0, n_compact = 0, n_wide = 0;
    for (size_t q = 0; q < P; ++q) {
        g_where = "puzzle " + std::to_string(q);
        // the reset state's legal mask: right, up, left, down in bounds and open
        uint32_t legal0 = 0;
        const int dx[4] = {1, 0, -1, 0}, dy[4] = {0, -1, 0, 1};
        for (int d = 0; d < 4; ++d) {
            const int x = (int)s.sx(q) + dx[d], y = (int)s.sy(q) + dy[d];
            if (x >= 0 && y >= 0 && x < (int)s.X(q) && y < (int)s.Y(q) && s.open_at(q, x, y)) legal0 |= 1u << d;
        }
        const uint32_t* inf = &p.info.v[4 * q];
        const uint32_t root_term = s.rooted(q) ? s.term(q, 0) : 0u;
        const uint4 info = make_uint4(inf[0], (inf[1] & 0x7FFFFu) | (root_term << 19), inf[2], s.cnt(q) | (legal0 << 16));
        CHECK(eq(h.info[q], info), "info row %08x %08x %08x %08x", h.info[q].x, h.info[q].y, h.info[q].z, h.info[q].w);
        const uint4 root = s.rooted(q) ? make_uint4(s.node(q, 0)[0], s.node(q, 0)[1], s.node(q, 0)[2], s.node(q, 0)[3])
                                       : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFu, 0u);
        CHECK(eq(h.root[q], root), "root row");
        const uint32_t sbit = s.sx(q) * pitch + s.sy(q), tbit = s.tx(q) * pitch + s.ty(q);
        uint64_t init = 0;
        uint4 row1 = make_uint4(0u, 0u, 0u, 0u);
        if (W == 1) {
            init = (p.open.v[q] & ~(1ull << sbit)) << pitch;
            row1 = make_uint4(sbit | (tbit << 8) | (info.y & 0xFFFF0000u), small ? (uint32_t)b8[q] : inf[2],
                              (s.cnt(q) ? s.cnt(q) - 1u : 0u) | (legal0 << 16), 0u);
        }
        CHECK(h.init[q] == init, "init %016llx", (unsigned long long)h.init[q]);
        CHECK(eq(h.row1[q], row1), "row1 %08x %08x %08x", h.row1[q].x, h.row1[q].y, h.row1[q].z);
        if (!small) continue;
        n_rootless += !s.rooted(q);
        // trie row: the root's record, the base, root S | solutions << 14 | max node << 17
        const uint32_t rootS = s.rooted(q) ? root_term << 15 : 0x10000u;
        const uint32_t tw = rootS | ((s.flags(q) & 1u) << 14) | ((s.cnt(q) ? s.cnt(q) - 1u : 0u) << 17);
        CHECK(h.trow[q].z == b8[q] && h.trow[q].z % 16 == 0, "trie8 base %u", h.trow[q].z);
        CHECK(h.trow[q].w == tw, "trow.w %08x, expected %08x", h.trow[q].w, tw);
        const uint2 rr = s.rooted(q) ? h.trie8[b8[q]] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        CHECK(h.trow[q].x == rr.x && h.trow[q].y == rr.y, "trow root record");
        const uint4 mrow = W == 1 ? make_uint4(row1.x, (uint32_t)init, (uint32_t)(init >> 32), q + 1 == P ? 0u : (uint32_t)q + 1u)
                                  : make_uint4(0u, 0u, 0u, 0u);
        CHECK(eq(h.mrow[q], mrow), "mrow");
        if (!s.rooted(q)) continue;
        for (uint32_t k = 0; k < s.cnt(q); ++k) {
            // the direction that reached node k: its parent's child field that names it
            uint32_t via = 4;
            if (k > 0)
                for (uint32_t d = 0; d < 4; ++d)
                    if (s.child(q, s.parent(q, k), d) == k) via = d;
            CHECK(k == 0 || via < 4, "node %u is no child of its parent", k);
            const uint2 rec = h.trie8[b8[q] + k];
            for (uint32_t d = 0; d < 4; ++d) {
                const uint32_t ch = s.child(q, k, d);
                uint32_t want = 0xFFFFu;
                if (ch != 0xFFFFu) want = ch | (s.term(q, ch) << 15);
                else if (k > 0 && d == (via ^ 2u)) want = s.parent(q, k) | (s.term(q, s.parent(q, k)) << 15);
                CHECK(field(rec, d) == want, "trie8 node %u field %u = %04x, expected %04x", k, d, field(rec, d), want);
                const uint2 la = h.trieg[4 * (b8[q] + k) + d];
                if (want == 0xFFFFu) CHECK(ones(la), "trieg node %u field %u not empty", k, d);
                else CHECK(eq(la, h.trie8[b8[q] + (want & 0x7FFFu)]), "trieg node %u field %u", k, d);
            }
        }
        if (W != 1) continue;
        // mixed table: 4-B records (8-bit fields) up to 127 nodes, else the 8-B records
        const bool compact = s.cnt(q) <= 127;
        (compact ? n_compact : n_wide) += 1;
        CHECK(h.trow4[q].z == b4[q] && h.trow4[q].z % 128 == 0, "trie4 base %u", h.trow4[q].z);
        auto f8 = [](uint32_t f) { return f == 0xFFFFu ? 0xFFu : (f & 0x7Fu) | ((f >> 15) << 7); };
        for (uint32_t k = 0; k < s.cnt(q); ++k) {
            const uint2 rec = h.trie8[b8[q] + k];
            if (compact) {
                for (uint32_t d = 0; d < 4; ++d)
                    CHECK(h.trie4[b4[q] + 4 * k + d] == f8(field(rec, d)), "trie4 node %u field %u", k, d);
            } else {
                CHECK(memcmp(&h.trie4[b4[q] + 8 * (size_t)k], &rec, 8) == 0, "trie4 8-B node %u", k);
            }
        }
    }
    g_where = "pool";
    for (size_t q = 0; q < P; ++q) {   // bit 13 marks exactly the compact puzzles
        if (!small || W != 1) break;
        const bool compact = s.rooted(q) && s.cnt(q) <= 127;
        CHECK(((h.trow4[q].w >> 13) & 1u) == (compact ? 1u : 0u), "trow4.w bit 13 of puzzle %zu", q);
        if (!s.rooted(q)) continue;
        const uint2 rr = h.trie8[b8[q]];
        if (compact) {
            auto f8 = [](uint32_t f) { return f == 0xFFFFu ? 0xFFu : (f & 0x7Fu) | ((f >> 15) << 7); };
            const uint32_t r4 = f8(field(rr, 0)) | (f8(field(rr, 1)) << 8) | (f8(field(rr, 2)) << 16) | (f8(field(rr, 3)) << 24);
            CHECK(h.trow4[q].x == r4 && h.trow4[q].y == 0xFFFFFFFFu, "trow4 root of compact puzzle %zu", q);
            CHECK((h.trow4[q].w & 0x180u) == (s.term(q, 0) << 7), "trow4 root S of puzzle %zu", q);
        } else {
            CHECK(h.trow4[q].x == rr.x && h.trow4[q].y == rr.y, "trow4 root of puzzle %zu", q);
        }
        CHECK((h.trow4[q].w >> 17) == s.cnt(q) - 1u && ((h.trow4[q].w >> 14) & 1u) == (s.flags(q) & 1u), "trow4.w of puzzle %zu", q);
    }
    if (small) {
        CHECK(h.trie8.size() == std::max<size_t>(end8, 1), "trie8 size %zu", h.trie8.size());
        CHECK(h.trieg.size() == 4 * h.trie8.size(), "trieg size");
        // records of no puzzle (line padding) are all ones
        std::vector<uint8_t> used(h.trie8.size(), 0);
        for (size_t q = 0; q < P; ++q)
            for (uint32_t k = 0; s.rooted(q) && k < s.cnt(q); ++k) used[b8[q] + k] = 1;
        for (size_t k = 0; k < used.size(); ++k)
            if (!used[k]) CHECK(ones(h.trie8[k]) && ones(h.trieg[4 * k]) && ones(h.trieg[4 * k + 3]), "padding record %zu", k);
        CHECK(h.mixed_pays == (h.trie8.size() * 8 > ((size_t)4 << 20)), "mixed_pays");
        CHECK(h.nodes8.size() == (W == 1 && h.mixed_pays ? P : 0), "nodes8");
        if (W == 1) CHECK(h.trie4.size() == end4 + 8, "trie4 ends 8 bytes past the last record: %zu vs %zu", h.trie4.size(), end4 + 8);
        else CHECK(h.trie4.empty() && h.trow4.empty(), "mixed tables are W = 1 only");
        CHECK(n_rootless == (uint32_t)p.get("expect_rootless", 0), "rootless puzzles %u", n_rootless);
        if (W == 1) CHECK((n_wide > 0) == (bool)p.get("expect_wide", 0) && n_compact > 0, "compact %u, 8-B %u tries", n_compact, n_wide);
    } else {
        CHECK(h.trie8.empty() && h.trieg.empty() && h.trow.empty() && h.trie4.empty() && !h.split_w, "no split tables");
    }
    // multi-word split kernel
    CHECK(h.split_w == (bool)p.get("expect_split_w", 0), "split_w %d", (int)h.split_w);
    if (W == 1 || pitch > 15) CHECK(!h.split_w, "split_w needs W > 1 and pitch <= 15");
    if (h.split_w) {
        const SplitGeom& g = h.sgeom;
        uint32_t xmax = 1, pts = 1;
        for (size_t q = 0; q < P; ++q) {
            xmax = std::max(xmax, s.X(q));
            pts = std::max(pts, s.X(q) * s.Y(q));
        }
        CHECK(g.P2 == pitch + 1, "P2");
        CHECK(g.B * 32 >= (xmax + 2) * g.P2 + 32 && g.B * 32 < (xmax + 2) * g.P2 + 64, "B %u", g.B);   // one spare dword
        CHECK(g.BS % 4 == 0 && g.BS >= g.B && g.BS < g.B + 4 && g.BS <= 4 * kBoardRegs, "BS %u", g.BS);
        CHECK(g.M == (p.tb ? (pts + 15) / 16 * 16 : 0u), "M %u (traceback %d)", g.M, (int)p.tb);
        CHECK(g.off_board == kLds.off_board && g.off_stack == g.off_board + 256 * g.BS, "board / stack offsets");
        CHECK(g.pair % 16 == 0 && g.pair >= g.off_stack + 64 * g.M && g.pair < g.off_stack + 64 * g.M + 16, "pair");
        CHECK(4 * (size_t)g.pair + kLds.fin_bytes <= kMaxDynLds, "LDS");
        CHECK(g.nbr_pos == ((2 * g.P2) | ((g.P2 - 1) << 8) | ((g.P2 + 1) << 24)), "nbr_pos");
        CHECK(h.mroww.size() == P && h.boardw.size() == P * g.BS, "sizes");
        std::vector<uint32_t> bw(P * g.BS, 0u);
        for (size_t q = 0; q < P; ++q) {
            CHECK(eq(h.mroww[q], make_uint4((s.sx(q) * g.P2 + s.sy(q)) | ((s.tx(q) * g.P2 + s.ty(q)) << 16), s.flags(q) & 7u, 0u, 0u)),
                  "mroww %zu", q);
            for (uint32_t x = 0; x < s.X(q); ++x)
                for (uint32_t y = 0; y < s.Y(q); ++y)
                    if (s.open_at(q, x, y) && !(x == s.sx(q) && y == s.sy(q))) {
                        const uint32_t d = (x + 1) * g.P2 + y;
                        bw[q * g.BS + d / 32] |= 1u << (d % 32);
                    }
        }
        CHECK(bw == h.boardw, "boardw: a bit exactly for each open point but the start");
    } else {
        CHECK(h.mroww.empty() && h.boardw.empty(), "no split_w tables");
    }
    bool ring = W == 1;
    for (size_t q = 0; q < P; ++q)
        if (s.X(q) * pitch > 57) ring = false;
    CHECK(h.ring_ok == ring, "ring_ok");
    if (p.meta.count("expect_ring_ok")) CHECK(ring == (bool)p.get("expect_ring_ok", 0), "ring_ok %d: the pool reaches the branch the test means", (int)ring);
}

void check_hash(const Pool& p, const HostPuzzleTables& h) {
    g_where = "table_hash";
    HostPuzzleTables again, other;
    CHECK(!build_puzzle_tables(&p.pt, p.W, p.pitch, p.tb, kLds, again) && again.table_hash == h.table_hash, "equal input");
    {
        Pool c = p;   // one bit of one open word
        c.open.v[c.open.v.size() / 2] ^= 1ull << 63;
        c.pt.open = c.open.ptr();
        CHECK(!build_puzzle_tables(&c.pt, p.W, p.pitch, p.tb, kLds, other) && other.table_hash != h.table_hash, "open word");
    }
    if (p.pt.num_nodes > 0) {
        Pool c = p;   // a depth word of the trie (w3: not validated, not in any table)
        c.trie.v[4 * (size_t)(p.pt.num_nodes - 1) + 3] ^= 0x100u;
        c.pt.trie = c.trie.ptr();
        CHECK(!build_puzzle_tables(&c.pt, p.W, p.pitch, p.tb, kLds, other) && other.table_hash != h.table_hash, "trie word");
    }
    CHECK(!build_puzzle_tables(&p.pt, p.W, p.pitch, !p.tb, kLds, other) && other.table_hash == h.table_hash, "traceback is no table fact");
}

void check_rules(const Pool& p, const HostPuzzleTables& hp) {
    g_where = "rules";
    const size_t P = hp.info.size();
    const int W = p.W;
    const size_t budget = (size_t)p.get("reg_entries", 1ll << 28);
    HostRuleTables r;
    const BuildError e = build_rule_tables(&p.rt, hp.info, W, budget, r);
    CHECK(!e, "rule tables rejected: %s", e.msg.c_str());
    if (e) return;
    const size_t S = (size_t)p.rt.num_shapes;
    CHECK(r.shape_range.size() == std::max<size_t>(S, 1) && r.inst_fc.size() == P, "range sizes");
    for (size_t k = 0; k < S; ++k)
        CHECK(r.shape_range[k].x == p.shape_first.v[k] && r.shape_range[k].x + r.shape_range[k].y == p.shape_first.v[k + 1], "shape %zu", k);
    CHECK(r.inst.size() == std::max<size_t>(1, p.rt.num_inst) && std::equal(p.inst.v.begin(), p.inst.v.begin() + p.rt.num_inst, r.inst.begin()), "inst copy");
    CHECK(r.shape_area.size() == std::max<size_t>(1, S) && std::equal(p.shape_area.v.begin(), p.shape_area.v.begin() + S, r.shape_area.begin()), "area copy");
    CHECK(r.shape_off.size() == 2 * std::max<size_t>(1, p.rt.num_offsets) &&
              std::equal(p.shape_off.v.begin(), p.shape_off.v.begin() + 2 * (size_t)p.rt.num_offsets, r.shape_off.begin()), "offset copy");
    CHECK(r.planes.size() == P * RP_COUNT * W, "plane count");
    bool area_ok = true;
    size_t host_fit = 0, entries = 0;
    bool cut = false, all = true;
    std::vector<uint2> items;
    for (size_t q = 0; q < P; ++q) {
        g_where = "rules of puzzle " + std::to_string(q);
        const uint32_t f = p.inst_first.v[q], n = p.inst_first.v[q + 1] - f;
        std::map<uint32_t, int64_t> net;   // cell bit -> net area
        std::set<uint32_t> shapes;
        uint32_t ylops = 0;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t en = p.inst.v[f + k], b = en & 0x3FFu, sh = en >> 11;
            const bool ylop = (en >> 10) & 1u;
            int64_t& v = net[b];
            v = std::max<int64_t>(-(1 << 20), std::min<int64_t>(1 << 20, v + (ylop ? -(int64_t)p.shape_area.v[sh] : p.shape_area.v[sh])));
            if (ylop) ++ylops;
            else shapes.insert(sh);
        }
        const bool hf = ylops > 16 || shapes.size() > 16;
        host_fit += hf;
        CHECK(r.inst_fc[q].x == f && (r.inst_fc[q].y & ~kHostFit) == n, "instance range");
        CHECK(((r.inst_fc[q].y & kHostFit) != 0) == hf, "kHostFit with %u ylops, %zu shapes", ylops, shapes.size());
        const uint64_t* d = &r.planes[q * RP_COUNT * W];
        for (uint32_t pl = 0; pl < RP_ABI; ++pl)
            for (int w = 0; w < W; ++w) {
                if (pl == RP_INST) continue;
                CHECK(d[pl * W + w] == p.planes.v[(q * RP_ABI + pl) * W + w], "plane %u word %d", pl, w);
            }
        for (uint32_t b = 0; b < 64u * W; ++b) {
            const bool has = net.count(b) != 0;
            CHECK(((d[RP_INST * W + b / 64] >> (b % 64)) & 1ull) == (has ? 1ull : 0ull), "RP_INST bit %u", b);
            const int64_t a = has ? net[b] : 0;
            if (a < -128 || a > 127) area_ok = false;
            uint32_t dec = 0;
            for (int k = 0; k < kAreaPlanes; ++k) dec |= (uint32_t)((d[(RP_AREA0 + k) * W + b / 64] >> (b % 64)) & 1ull) << k;
            CHECK(dec == ((uint32_t)a & 0xFFu), "area planes of bit %u decode to %u, net area %lld", b, dec, (long long)a);
            if (a >= -128 && a <= 127) CHECK((int8_t)dec == a, "signed area of bit %u", b);
        }
        // region-code table: 2^cells entries of 4 bits (at least 8), contiguous, until the budget
        const uint32_t X = p.info.v[4 * q] & 0xFFu, Y = (p.info.v[4 * q] >> 8) & 0xFFu;
        const uint32_t cells = ((X - 1) / 2) * ((Y - 1) / 2);
        uint32_t want = kNoRegTab;
        if (cells <= 12 && !cut) {
            const size_t ent = std::max<size_t>(8, (size_t)1 << cells);
            if (entries + ent > budget) cut = true;
            else {
                want = (uint32_t)entries;
                for (uint32_t g = 0; g < ent / 8; ++g) items.push_back(make_uint2((uint32_t)q, g));
                entries += ent;
            }
        }
        all &= want != kNoRegTab;
        CHECK(r.reg_off[q] == want, "reg_off %u, expected %u", r.reg_off[q], want);
    }
    g_where = "rules";
    CHECK(r.area_ok == area_ok && area_ok == (bool)p.get("expect_area_ok", 1), "area_ok %d", (int)r.area_ok);
    CHECK(r.host_fit_puzzles == host_fit && host_fit == (size_t)p.get("expect_host_fit", 0), "host-fit puzzles %zu", r.host_fit_puzzles);
    CHECK(r.reg_words == entries / 8 && entries <= budget, "region table words %zu", r.reg_words);
    CHECK(r.items.size() == items.size() && std::equal(items.begin(), items.end(), r.items.begin(), [](uint2 a, uint2 b) { return eq(a, b); }), "work list");
    CHECK(r.tab_all == all && all == (bool)p.get("expect_tab_all", 1), "tab_all %d", (int)r.tab_all);
    const std::vector<uint64_t> rows = build_rule_rows(r, hp.info, W);
    const size_t RW = 10 * W + 2;
    CHECK(rows.size() == P * RW, "rows size");
    const uint32_t base[10] = {RP_CELLS, RP_LATTICE, RP_GAPS, RP_DOTS, RP_TRI, RP_TRI0, RP_TRI1, RP_TRI2, RP_NOTFIRST, RP_NOTLAST};
    for (size_t q = 0; q < P && rows.size() == P * RW; ++q) {
        for (int k = 0; k < 10; ++k)
            for (int w = 0; w < W; ++w)
                CHECK(rows[q * RW + k * W + w] == p.planes.v[(q * RP_ABI + base[k]) * W + w], "row %zu plane %d", q, k);
        const uint32_t n = p.inst_first.v[q + 1] - p.inst_first.v[q];
        const uint32_t cf = (n & 0x7Fu) | ((r.inst_fc[q].y & kHostFit) ? 0x80u : 0u);
        CHECK(rows[q * RW + 10 * W] == ((uint64_t)r.reg_off[q] | ((uint64_t)p.inst_first.v[q] << 32)), "row %zu offsets", q);
        CHECK(rows[q * RW + 10 * W + 1] == ((uint64_t)hp.info[q].x | ((uint64_t)((hp.info[q].y & 0xFFFFFFu) | (cf << 24)) << 32)), "row %zu info", q);
    }
}

int run_check(const std::string& dir) {
    const Pool p = load_pool(dir);
    g_where = dir;
    HostPuzzleTables h;
    const BuildError e = build_puzzle_tables(&p.pt, p.W, p.pitch, p.tb, kLds, h);
    CHECK(!e, "puzzle table rejected: %s", e.msg.c_str());
    if (e) return 1;
    check_puzzles(p, h);
    check_hash(p, h);
    if (p.planes.present) check_rules(p, h);
    return 0;
}

void run_reject(const std::string& dir) {
    const Pool p = load_pool(dir);
    HostPuzzleTables h;
    BuildError e = build_puzzle_tables(&p.pt, p.W, p.pitch, p.tb, kLds, h);
    if (!e && p.get("rules", 0)) {
        HostRuleTables r;
        e = build_rule_tables(p.get("null_rules", 0) ? nullptr : &p.rt, h.info, p.W, (size_t)1 << 28, r);
    }
    printf("%d|%s\n", e.code, e.msg.c_str());
}

void run_hostfits() {
    g_where = "hostfits";
    std::vector<uint4> tab;
    std::vector<std::pair<uint32_t, uint64_t>> keys;
    uint64_t x = 88172645463325252ull;
    size_t used = 0;
    for (int k = 0; k < 9000; ++k) {   // 2^12 slots hold 2048: two growths
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        const uint32_t q = (uint32_t)(x >> 40) % 1000u;
        const uint64_t rm = x & ((1ull << 49) - 1);
        hostfits_grow(tab, used + 1);
        if (hostfits_insert(tab, q, rm, (uint32_t)(x >> 63))) {
            keys.push_back({q, rm | (x >> 63 << 63)});
            ++used;
        }
        CHECK(2 * used <= tab.size() && (tab.size() & (tab.size() - 1)) == 0, "load factor at %zu of %zu", used, tab.size());
    }
    CHECK(tab.size() == (size_t)1 << 15 && used > 8900, "grown from 2^12 to %zu slots for %zu answers", tab.size(), used);
    for (const auto& kv : keys) {
        const uint64_t rm = kv.second & ~(1ull << 63);
        const uint32_t mask = (uint32_t)tab.size() - 1;
        int found = -1;
        for (uint32_t s = hostfit_slot(kv.first, rm, mask), n = 0; n < tab.size(); s = (s + 1) & mask, ++n) {
            const uint4 en = tab[s];
            if (!(en.w & 2u)) break;
            if (en.x == (uint32_t)rm && en.y == (uint32_t)(rm >> 32) && en.z == kv.first) {
                found = (int)(en.w & 1u);
                break;
            }
        }
        CHECK(found == (int)(kv.second >> 63), "entry (%u, %llx) found as %d", kv.first, (unsigned long long)rm, found);
        CHECK(!hostfits_insert(tab, kv.first, rm, 0u), "a duplicate is refused");
    }
    // xcd_hot_bytes: per group of workgroups b, b + 8, ... the distinct puzzles its envs play
    g_where = "xcd_hot_bytes";
    std::vector<uint32_t> nodes(37), q(2048 + 256);
    for (size_t k = 0; k < nodes.size(); ++k) nodes[k] = 10 + 7 * (uint32_t)k;
    for (size_t i = 0; i < q.size(); ++i) q[i] = (uint32_t)((i * 2654435761u) >> 7) % 37u;
    size_t want = 0;
    for (uint32_t g = 0; g < 8; ++g) {
        std::set<uint32_t> hot;
        for (size_t i = 0; i < q.size(); ++i)
            if ((i / 256) % 8 == g)
                for (uint32_t k = 0; k < kHotWalk; ++k) hot.insert((q[i] + k) % 37u);
        size_t b = 0;
        for (uint32_t u : hot) b += 8 * (size_t)nodes[u];
        want = std::max(want, b);
    }
    CHECK(xcd_hot_bytes(nodes, q.data(), (uint32_t)q.size()) == want, "largest group's bytes");
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "check") {
        for (int k = 2; k < argc; ++k) {
            const int before = g_fail;
            run_check(argv[k]);
            if (g_fail == before) printf("ok %s\n", argv[k]);
        }
    } else if (mode == "reject") {
        for (int k = 2; k < argc; ++k) run_reject(argv[k]);
    } else if (mode == "hostfits") {
        run_hostfits();
        if (!g_fail) printf("ok hostfits\n");
    } else {
        fprintf(stderr, "usage: tables_main check|reject DIR... | hostfits\n");
        return 2;
    }
    return g_fail ? 1 : 0;
}
