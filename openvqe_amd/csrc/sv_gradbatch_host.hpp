// sv_gradbatch_host.hpp — the launch geometry of k_sparse_grad_batch (sv_sparse.hpp), host only: no HIP header, g++ compiles it alone
// (tests/cpu/gradbatch_plan_check.cpp).  gradbatch_host.inc launches what plan() answers; tests/gradbatch_cases.py restates the rule.
//
// A candidate is (nw, stage): nw in {1, 2, 4, 8} waves per workgroup, the op records and pair words staged in LDS or read from global
// memory; its bytes are sp_grad_batch_lds(A, nw, stage).bytes.  It is ADMISSIBLE when they are at most LDS_BUDGET.  Among the admissible
// candidates the one with the most RESIDENT WAVES per CU wins — the kernel is bound by LDS latency, and other waves are what hides it:
//     resident workgroups per CU = min(floor(LDS_CU / bytes), waves_cu(stage) / nw),   resident waves = that x nw
// A CU holds 160 KiB of LDS.  The second bound is the register file's: the compiler's resource-usage remarks give the staged instances
// 72 VGPRs (7 waves per SIMD, 28 per CU) and the unstaged ones 73 (6 per SIMD, 24 per CU), for every nw; only small programs meet it.
// Ties prefer the staged form, then the smaller nw (fewer waves idle at the barrier and in the last trip of a batch that is no multiple
// of nw).
// Option "grad_batch_waves" restricts the candidates to one nw (where none of them is admissible, the choice is the automatic one);
// "grad_batch_workgroups" caps the grid.
//     workgroups = min(ceil(B / nw), CUs x resident workgroups per CU, the cap when set), at least 1
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "sv_sparse_layout.hpp"

namespace ovqe {
namespace gradbatch {

constexpr size_t LDS_BUDGET = 150 * 1024;   // LDS_WG_BUDGET of ovqe_sv.hip (asserted there)
constexpr size_t LDS_CU = 160 * 1024;       // LDS_WG_MAX
constexpr int waves_cu(bool stage) { return stage ? 28 : 24; }   // 4 SIMDs x the occupancy of the instances (profiles/gradient_batch)

struct Plan {
    bool ok = false;      // false: no candidate is admissible (nothing else is set)
    int nw = 0;
    bool stage = false;
    int per_cu = 0;       // resident workgroups per CU
    int64_t workgroups = 0;
    size_t lds = 0;
};

inline bool valid_waves(int64_t v) { return v == 1 || v == 2 || v == 4 || v == 8; }

// the unstaged one-wave layout within the budget: what makes a program eligible at all (the criterion of the single call's one-wave forms)
inline bool eligible(const SparseArgs &A) { return sp_grad_batch_lds(A, 1, false).bytes <= LDS_BUDGET; }

// the rule over any per-wave layout (k_sparse_spread_batch plans with it on its own: sv_spread_host.hpp): bytes_of(nw, stage) are a
// candidate's bytes, waves_of(stage) the waves a CU holds of the instances
template <class Bytes, class WavesCu>
inline Plan plan_rule(Bytes bytes_of, WavesCu waves_of, int64_t B, int opt_waves, int64_t opt_workgroups, int cus) {
    // a forced nw none of whose forms is admissible: the automatic choice (a tuning knob does not send a program to the row-by-row path)
    if (valid_waves(opt_waves) && bytes_of(opt_waves, false) > LDS_BUDGET) opt_waves = 0;
    Plan best;
    int best_waves = -1;
    for (bool stage : {true, false}) {
        for (int nw : {1, 2, 4, 8}) {
            if (valid_waves(opt_waves) && nw != opt_waves) continue;
            const size_t bytes = bytes_of(nw, stage);
            if (bytes > LDS_BUDGET) continue;
            const int per_cu = (int)std::min<size_t>(LDS_CU / std::max<size_t>(bytes, 1), (size_t)(waves_of(stage) / nw));
            const int waves = per_cu * nw;
            if (waves <= best_waves) continue;   // visited in the order of the tie-break: a later candidate must be strictly better
            best_waves = waves;
            best.ok = true;
            best.nw = nw;
            best.stage = stage;
            best.per_cu = per_cu;
            best.lds = bytes;
        }
    }
    if (!best.ok) return best;
    int64_t wgs = std::min<int64_t>((B + best.nw - 1) / best.nw, (int64_t)std::max(cus, 1) * best.per_cu);
    if (opt_workgroups > 0) wgs = std::min(wgs, opt_workgroups);
    best.workgroups = std::max<int64_t>(wgs, 1);
    return best;
}

inline Plan plan(const SparseArgs &A, int64_t B, int opt_waves, int64_t opt_workgroups, int cus) {
    return plan_rule([&](int nw, bool stage) { return sp_grad_batch_lds(A, nw, stage).bytes; }, [](bool stage) { return waves_cu(stage); }, B,
                     opt_waves, opt_workgroups, cus);
}

}  // namespace gradbatch
}  // namespace ovqe
