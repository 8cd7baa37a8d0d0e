// exact_fit_main — the exact-fit search of csrc/sparc_rules.hpp on the CPU, as a stand-alone
// program (tests/test_exact_fit_host.py builds it with -fsanitize=address,undefined and runs it as
// a child process; no GPU, no library).
//
// Input (argv[1], text): the packed rule table of a pool and a list of searches,
//   pitch P / puzzles N, then N lines "X Y first count" / inst M, then M values /
//   shapes S, then S + 1 offsets / offsets O, then O pairs "dx dy" / searches K, then K lines "q rm".
// Per search it runs exact_fit in the GPU's instantiation <uint32_t, kFitYlops, kFitShapes,
// kFitPlanes> (cap 0 for a puzzle past those lists, as fit_in gives a kHostFit puzzle) and in the
// host's <uint64_t, kHostFitMax, kHostFitMax, kHostFitPlanes>, without a cap and at caps around the
// search's own node count (the smallest cap at which it finishes, found by bisection), and prints
//   S q rm flagged answer32 nodes32 answer64 nodes64
//   C cap result32 result64          (one line per cap tried; -1: not finished)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sparc_rules.hpp"

using namespace sparc;

namespace {
constexpr int W = 4;

struct Pool {
    uint32_t pitch = 0;
    std::vector<uint32_t> X, Y, first, count, inst;
    std::vector<uint2> shape_range;
    std::vector<int8_t> off;
};

bool expect(FILE* f, const char* word, long long& v) {
    char w[32];
    return fscanf(f, "%31s %lld", w, &v) == 2 && std::string(w) == word;
}

struct Search {
    const Pool& p;
    FitIn fin;
    BB<W> Rc;
    uint64_t rm;
    bool flagged;

    Search(const Pool& pool, uint32_t q, uint64_t m) : p(pool), rm(m) {
        fin = FitIn{p.inst.data(), p.shape_range.data(), p.off.data(), p.first[q], p.count[q],
                    (p.X[q] - 1) / 2, (p.Y[q] - 1) / 2, 0u};
        Rc = BB<W>::zero();
        for (uint32_t b = 0; b < fin.CX * fin.CY; ++b)
            if ((rm >> b) & 1ull) Rc.set((2 * (b / fin.CY) + 1) * p.pitch + 2 * (b % fin.CY) + 1);
        // the loader's flag (build_rule_tables): more ylops or distinct poly shapes than the GPU's lists
        int ny = 0;
        std::vector<uint32_t> ds;
        for (uint32_t k = 0; k < fin.count; ++k) {
            const uint32_t e = p.inst[fin.first + k];
            if ((e >> 10) & 1u) { ++ny; continue; }
            bool seen = false;
            for (uint32_t s : ds) seen |= s == (e >> 11);
            if (!seen) ds.push_back(e >> 11);
        }
        flagged = ny > kFitYlops || (int)ds.size() > kFitShapes;
    }
    int gpu(uint32_t cap) const { return exact_fit<W, uint32_t>(fin, Rc, rm, flagged ? 0u : cap); }
    int host(uint64_t cap) const {
        return exact_fit<W, uint64_t, kHostFitMax, kHostFitMax, kHostFitPlanes>(fin, Rc, rm, cap);
    }
    // the smallest cap at which the search finishes
    template <class F>
    static uint64_t nodes(F&& run) {
        uint64_t hi = 1;
        while (run(hi) < 0) hi *= 2;
        uint64_t lo = hi / 2;   // run(lo) < 0 (or lo == 0)
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (run(mid) < 0) lo = mid; else hi = mid;
        }
        return hi;
    }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    Pool p;
    long long v, n;
    if (!expect(f, "pitch", v)) return 3;
    p.pitch = (uint32_t)v;
    if (!expect(f, "puzzles", n)) return 3;
    for (long long i = 0; i < n; ++i) {
        unsigned a, b, c, d;
        if (fscanf(f, "%u %u %u %u", &a, &b, &c, &d) != 4) return 3;
        p.X.push_back(a), p.Y.push_back(b), p.first.push_back(c), p.count.push_back(d);
    }
    if (!expect(f, "inst", n)) return 3;
    for (long long i = 0; i < n; ++i) {
        unsigned a;
        if (fscanf(f, "%u", &a) != 1) return 3;
        p.inst.push_back(a);
    }
    if (!expect(f, "shapes", n)) return 3;
    std::vector<uint32_t> sf;
    for (long long i = 0; i <= n; ++i) {
        unsigned a;
        if (fscanf(f, "%u", &a) != 1) return 3;
        sf.push_back(a);
    }
    for (long long i = 0; i < n; ++i) p.shape_range.push_back(make_uint2(sf[i], sf[i + 1] - sf[i]));
    if (!expect(f, "offsets", n)) return 3;
    for (long long i = 0; i < 2 * n; ++i) {
        int a;
        if (fscanf(f, "%d", &a) != 1) return 3;
        p.off.push_back((int8_t)a);
    }
    if (sf.back() != (uint32_t)n) return 3;
    if (!expect(f, "searches", n)) return 3;
    for (long long i = 0; i < n; ++i) {
        unsigned q;
        uint64_t rm;
        if (fscanf(f, "%u %" SCNx64, &q, &rm) != 2 || q >= p.X.size()) return 3;
        const Search s(p, q, rm);
        const int a64 = s.host(~0ull);
        const uint64_t n64 = Search::nodes([&](uint64_t c) { return s.host(c); });
        int a32 = -1;
        uint64_t n32 = 0;
        if (!s.flagged) {
            a32 = s.gpu(~0u);
            n32 = Search::nodes([&](uint64_t c) { return s.gpu((uint32_t)c); });
        }
        printf("S %u %" PRIx64 " %d %d %" PRIu64 " %d %" PRIu64 "\n", q, rm, (int)s.flagged, a32, n32, a64, n64);
        const uint64_t caps[] = {0, 1, n64 / 2, n64 - 1, n64, n64 + 1, 2 * n64 + 3, 1000 * n64};
        for (uint64_t c : caps)
            printf("C %" PRIu64 " %d %d\n", c, s.gpu((uint32_t)c), s.host(c));
    }
    fclose(f);
    return 0;
}
