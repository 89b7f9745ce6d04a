// sv_spread_host.hpp — launch geometry and eligibility of k_sparse_spread_batch (sv_sparse.hpp), host only: no HIP header, g++ compiles
// it alone (tests/cpu/spread_plan_check.cpp).  spread_host.inc launches what plan() answers; tests/spread_cases.py restates both rules.
//
// GEOMETRY.  gradbatch::plan_rule (sv_gradbatch_host.hpp) on the larger layout sp_spread_batch_lds — three state arrays per wave — under
// the same options "grad_batch_waves" and "grad_batch_workgroups", with the register bound of THIS kernel's instances: the compiler's
// resource-usage remarks give the staged instances 73 VGPRs (6 waves per SIMD, 24 per CU) and the unstaged ones 71 (7 per SIMD, 28 per
// CU), for every nw, and no scratch (profiles/spread) — the other way round from k_sparse_grad_batch's 72 / 73.
//
// ELIGIBILITY.  The compact program keeps the Hamiltonian RESTRICTED to the support, and of its terms those with an even number of Y
// (build_sparse_program).  On the real state psi that is exact for <psi|H|psi> and its gradient: what leaves the support meets zeros of
// psi, and <psi|P|psi> of a term with an odd number of Y is zero.  It is not exact for ||H psi||^2, which counts every component of
// H psi.  exactness() decides when the restricted entries ARE H on the support:
//   odd_y   a term with an odd number of Y and a non-zero coefficient exists;
//   leak    for an x-group g and a support state a whose partner a ^ x_g is outside the support, |D_g| > the group's `tiny`, D_g the
//           signed sum of the group's even-Y coefficients at that pair.  tiny = 64 eps sum_t |c_t| is the residue rule of
//           group_coeff_snap (sv_kernels.hpp): number-conserving Hamiltonians cancel on such pairs to 1e-17 .. 3e-16, not to 0.0.
// With neither, H maps the span of the support into itself and k_sparse_spread_batch's second pass over the entries is H^2 psi.
#pragma once
#include <cmath>
#include <vector>

#include "sv_cover_host.hpp"
#include "sv_gradbatch_host.hpp"

namespace ovqe {
namespace spread {

constexpr int waves_cu(bool stage) { return stage ? 24 : 28; }   // 4 SIMDs x the occupancy of the instances (profiles/spread)

// one wave's three-array region within the budget
inline bool fits(const SparseArgs &A) { return sp_spread_batch_lds(A, 1, false).bytes <= gradbatch::LDS_BUDGET; }

inline gradbatch::Plan plan(const SparseArgs &A, int64_t B, int opt_waves, int64_t opt_workgroups, int cus) {
    return gradbatch::plan_rule([&](int nw, bool stage) { return sp_spread_batch_lds(A, nw, stage).bytes; }, [](bool stage) { return waves_cu(stage); },
                                B, opt_waves, opt_workgroups, cus);
}

struct Exactness {
    bool odd_y = false, leak = false;
};

// support: the basis states of the compact program; in_support(a): whether a is one of them
template <class InSupport>
Exactness exactness(const std::vector<HGroup> &groups, const std::vector<HTerm> &terms, const std::vector<uint64_t> &support, InSupport in_support) {
    Exactness out;
    for (const HGroup &g : groups) {
        for (int t = g.t0; t < g.t1; ++t)
            if ((__builtin_popcountll(g.x & terms[t].z) & 1) && (terms[t].cr != 0.0 || terms[t].ci != 0.0)) out.odd_y = true;
        if (!g.x || out.leak) continue;
        for (const uint64_t a : support) {
            const uint64_t b = a ^ g.x;
            if (in_support(b)) continue;
            double d = 0.0;
            for (int t = g.t0; t < g.t1; ++t) {
                const HTerm &ht = terms[t];
                if (__builtin_popcountll(g.x & ht.z) & 1) continue;
                d += (__builtin_popcountll(b & ht.z) & 1) ? -ht.cr : ht.cr;
            }
            if (std::fabs(d) > g.tiny) {
                out.leak = true;
                break;
            }
        }
    }
    return out;
}

// why a call is served row by row (ovqe_spread_info [10])
enum Why : int { WHY_NONE = 0, WHY_NO_COMPACT = 1, WHY_LDS = 2, WHY_LEAK = 3, WHY_ODD_Y = 4 };

}  // namespace spread
}  // namespace ovqe
