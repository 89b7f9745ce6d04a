// sv_hessian_host.hpp — host-side plan of the exact energy Hessian (kernel: k_sparse_hessian in sv_sparse.hpp; handle section:
// hessian_host.inc; entry points ovqe_energy_hessian / ovqe_hessian_info: abi_hessian.inc).  Host-only: no HIP, no handle types — g++
// compiles it alone (tests/cpu/hessian_plan_check.cpp replays its tables the way the kernel indexes them and compares with a dense
// simulation).
//
// THE MATHEMATICS.  Rotation r has the angle phi_r = coeff_r theta[pidx_r] + phi0_r, psi_r = U_r ... U_1 |hf>, E = <psi_R|H|psi_R>.  The
// adjoint gradient reads w_r = 2 Im <lambda_r|P_r|psi_r> on the states after rotation r, walking lambda_{r-1} = U_r^+ lambda_r and
// psi_{r-1} = U_r^+ psi_r backwards from lambda_R = H psi_R; dE/dtheta_k = sum_{r in k} coeff_r w_r.  That pass, differentiated in the
// direction b (forward over reverse), with a dot for d / dtheta_b:
//   start            psi'_R = T_b (the tangent of the metric),   lambda'_R = H T_b
//   at rotation r    w'_r = 2 Im( <lambda'_r|P_r|psi_r> + <lambda_r|P_r|psi'_r> )                      (before it is un-applied)
//   un-apply         psi'_{r-1}    = U_r^+ psi'_r    + [pidx_r = b] coeff_r (i P_r) psi_{r-1}
//                    lambda'_{r-1} = U_r^+ lambda'_r + [pidx_r = b] coeff_r (i P_r) lambda_{r-1}
//   row b            d2E / dtheta_b dtheta_k = sum_{r in k} coeff_r w'_r
// COMPACT REAL FORM (path 1; the program is the metric's, sv_metric_host.hpp).  A pair (i, j) with table entry (c, s) and sign sigma is
// the Givens step G: u' = c u + sigma s v, v' = c v - sigma s u; dG / dphi = G J = J G with J = [[0, sigma], [-sigma, 0]].  On real vectors
// E = psi^T H psi with H the real part of the Hamiltonian restricted to the support, the pair weight of the gradient is
// g = lambda_i psi_j - lambda_j psi_i (added to w[e] with the sign sigma, dE / dphi_e = 2 w[e]), and with d = coeff_e for an entry of
// parameter b, 0 otherwise:
//   forward          t' = G t + d J psi'                                   (k_sparse_metric's step)
//   weight           g' = mu_i psi_j - mu_j psi_i + lambda_i t_j - lambda_j t_i      (mu = lambda'; on the states before un-applying)
//   un-apply         psi = G^T psi', lambda = G^T lambda', t = G^T t', mu = G^T mu', then the injection -d J of the un-applied states:
//                    t_i -= d sigma psi_j,  t_j += d sigma psi_i,  mu_i -= d sigma lambda_j,  mu_j += d sigma lambda_i
// Below the first op that holds an entry of parameter b the tangent t is exactly zero: the kernel drops it there and keeps the mu term.
// The raw matrix M (row b from workgroup b) is symmetric to rounding only; the call returns (M + M^T) / 2 and reports max |M - M^T|.
#pragma once
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "sv_cover_host.hpp"
#include "sv_metric_host.hpp"
#include "sv_sparse_layout.hpp"

namespace ovqe {
namespace hessian {

using Entry = SpEntry;   // the record k_sparse_grad's lambda loop reads (sv_sparse_layout.hpp)
struct Restricted {
    std::vector<Entry> entries;
    double constant = 0.0;   // the caller's constant plus the identity terms: added to E, never an entry
};

// Re H on `support` (compact index k <-> basis state support[k]) from the grouped terms (i^ny folded into cr + i ci, build_groups):
// <a ^ x| c P |a> = (cr + i ci) (-1)^{parity(a & z)}; a string with an odd number of Y has an imaginary element and drops out.
// false: more than `max_entries` entries
inline bool restrict_hamiltonian(const std::vector<uint64_t> &support, const std::vector<HGroup> &groups, const std::vector<HTerm> &terms,
                                 double constant, size_t max_entries, Restricted *out) {
    Restricted &R = *out;
    R = Restricted();
    R.constant = constant;
    const int m = (int)support.size();
    std::unordered_map<uint64_t, int> id;
    for (int k = 0; k < m; ++k) id.emplace(support[(size_t)k], k);
    for (const HGroup &g : groups) {
        const uint64_t x = g.x;
        if (x == 0) {
            for (int t = g.t0; t < g.t1; ++t)
                if (terms[(size_t)t].z == 0) R.constant += terms[(size_t)t].cr;
        }
        for (int k = 0; k < m; ++k) {
            const uint64_t a = support[(size_t)k];
            int kb = k;
            if (x) {
                const auto it = id.find(a ^ x);
                if (it == id.end() || it->second <= k) continue;   // the partner outside the support, or the pair met from its other end
                kb = it->second;
            }
            double d = 0.0;
            for (int t = g.t0; t < g.t1; ++t) {
                const HTerm &ht = terms[(size_t)t];
                if ((__builtin_popcountll(x & ht.z) & 1) || (x == 0 && ht.z == 0)) continue;
                d += metric::parity64(a & ht.z) ? -ht.cr : ht.cr;
            }
            if (d == 0.0) continue;
            if (R.entries.size() >= max_entries) return false;
            R.entries.push_back(Entry{(uint32_t)k | ((uint32_t)kb << 12), 0u, x ? 2.0 * d : d});
        }
    }
    return true;
}

// the streaming path's workspace: two stores in the metric's layout (columns psi, T_1 .. T_K and their images under H), the slab sums of
// one weight reduction ([nslabs][wpad] doubles, slabs of slab_rows rows: at most 256 of them, at least four rows each) and the weight
// records ([nrec][wpad] doubles: the energy and one per parameterised rotation)
struct Streaming {
    int64_t slab_rows = 0, nslabs = 0;
    size_t store_bytes = 0, part_bytes = 0, w_bytes = 0, bytes = 0;
};
inline Streaming streaming_layout(int64_t rows, int64_t K, int64_t nrec) {
    const metric::Store st = metric::store_layout(rows, K, false);
    Streaming s;
    s.slab_rows = std::max<int64_t>(4, (rows + 255) / 256);
    s.nslabs = (rows + s.slab_rows - 1) / s.slab_rows;
    s.store_bytes = st.bytes;
    s.part_bytes = (size_t)s.nslabs * (size_t)st.wpad * sizeof(double);
    s.w_bytes = (size_t)nrec * (size_t)st.wpad * sizeof(double);
    s.bytes = 2 * s.store_bytes + s.part_bytes + s.w_bytes;
    return s;
}

}  // namespace hessian
}  // namespace ovqe
