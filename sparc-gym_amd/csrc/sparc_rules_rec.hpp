// sparc_rules_rec.hpp — rule audit of state records (device code): what a tree search asks about
// the nodes of a frontier, M records -> M rule-bit words (+ region maps and fit masks).
//
// Record j gets the audit k_rules gives an env that k_restore filled from it (_validate_rules,
// SPaRC_Gym.py:941-950), in one launch and without an env: the context supplies the puzzle and
// rule tables and the pitch only; no env state and no per-env exact-fit memo (Ctx::r_memo is
// keyed to envs, and M is not num_envs) is read or written.
//
//   One lane per record, 256-lane workgroups.  A lane reads its record as 16-B pieces and only
//   the pieces the audit needs: the first (pos, aux, step, pid) and those that hold the visited
//   words; the direction stack is never read (32 of the 48 bytes of a W = 1 traceback record).
//   The audit is the project's own (puzzle_rules, audit / audit_r of sparc_rules.hpp) on the
//   record's board and agent position, with the record index as the FitQueue output index and
//   the HostFits table applied as in k_rules.
//   The exact-fit memo is NoMemo: a lane audits one state, whose regions are distinct cell masks,
//   so a lane-local memo that starts empty could never hit; it would only cost registers.
//   TABLE_ONLY (W = 1, every puzzle has a region-code table, host-checked): audit_r's table-only
//   form, with no region check and no exact-fit search compiled in; it writes bits only.
//
// A record is checked before anything is indexed with it: the conditions of k_restore
// (expand_record_ok) and pid below the rule table's puzzle count.  A record that fails gets bits
// 0, fit 0, keeps its region row all 0xFF, and raises kErrSnapshot (kErrRuleTable for the rule
// table's bound, as k_rules does); every other record is unaffected.
#pragma once
#include "sparc_expand.hpp"
#include "sparc_rules.hpp"

namespace sparc {

// 16-B pieces of a record that hold its scalars and its visited board
template <int W>
constexpr int rules_rec_pieces() { return (4 + 2 * W + 3) / 4; }

// bits[j], region[j][64 W], fit[j] <- audit(record j) for j < M; `pieces`: 16-B pieces per record
// (the header's record_bytes / 16).  region and fit may be NULL; TABLE_ONLY ignores them.
template <int W, bool TABLE_ONLY>
__global__ void __launch_bounds__(kSnapBlock) k_rules_rec(Params p, RulesTab rt, const uint4* __restrict__ rec,
                                                          uint32_t pieces, uint32_t M, uint16_t* __restrict__ bits,
                                                          uint8_t* __restrict__ region, uint64_t* __restrict__ fit) {
    static_assert(!TABLE_ONLY || W == 1, "the table-only audit is the one-word one");
    constexpr int kRead = rules_rec_pieces<W>();
    const uint32_t j = blockIdx.x * kSnapBlock + threadIdx.x;
    if (j >= M) return;
    const uint4* pc = rec + (size_t)j * pieces;
    uint32_t w[4 * kRead];
#pragma unroll
    for (int k = 0; k < kRead; ++k) {
        const uint4 v = pc[k];
        w[4 * k] = v.x;
        w[4 * k + 1] = v.y;
        w[4 * k + 2] = v.z;
        w[4 * k + 3] = v.w;
    }
    uint8_t* ro = nullptr;
    if constexpr (!TABLE_ONLY) {
        ro = region ? region + (size_t)j * 64 * W : nullptr;
        if (ro)
            for (int k = 0; k < 64 * W; ++k) ro[k] = 0xFF;
    }
    const uint32_t pos = w[0], q = w[3];
    uint32_t out = 0;
    uint64_t fit_ok = 0;
    if (!expand_record_ok(p.tab, pos, w[1], q)) {
        atomicOr(p.err, (int)kErrSnapshot);
    } else if (q >= rt.num_puzzles) {
        atomicOr(p.err, (int)kErrRuleTable);
    } else {
        BB<W> vis;
#pragma unroll
        for (int k = 0; k < W; ++k) vis.w[k] = w[4 + 2 * k] | ((uint64_t)w[4 + 2 * k + 1] << 32);
        const uint32_t x = pos & 0xFFu, y = (pos >> 8) & 0xFFu;
        const PuzzleRules<W> pr = puzzle_rules<W>(p, rt, q);
        if constexpr (TABLE_ONLY) {
            out = audit_r<1, NoMemo, true>(p, rt, pr, vis, x == pr.tx && y == pr.ty, nullptr, nullptr).bits;
        } else {
            const RuleOut<W> r = audit<W, NoMemo>(p, rt, pr, vis, x, y, ro, nullptr, j);
            out = r.bits;
            fit_ok = r.fit_ok;
        }
    }
    bits[j] = (uint16_t)out;
    if constexpr (!TABLE_ONLY)
        if (fit) fit[j] = fit_ok;
}

}  // namespace sparc
