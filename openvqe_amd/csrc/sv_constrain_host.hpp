// sv_constrain_host.hpp — the ONE rule that restricts a grouped Pauli sum to the support of a compact program, and the limits of the
// observables a handle holds beside its Hamiltonian (constrain_host.inc), host only: no HIP header, g++ compiles it alone
// (tests/cpu/restrict_check.cpp).  build_sparse_program restricts the Hamiltonian with it, constrain_host.inc every observable.
//
// THE RULE.  For a Hermitian sum O = sum_t c_t P_t with real c_t, grouped by x mask, and a support S of basis states, the entries are
//     diagonal (x = 0):    (k, k, D(a_k))                     for every a_k in S,
//     off-diagonal:        (k, k', 2 D(a_k ^ x))              for every a_k in S with the highest bit of x clear whose partner
//                                                             a_k' = a_k ^ x is in S — the pair counted once,
// where D(b) = sum over the group's terms with an EVEN number of Y of +-c_t, the sign the parity of b & z_t (c_t with i^ny folded in:
// build_groups), and entries with D == 0.0 are dropped.  Groups in their stored order, support states in the order given.
// EXACTNESS.  On a REAL state psi that is zero off S, <psi|O|psi> and the vector the backward walk contracts with, the part of O psi on
// S, come out exactly: a partner outside S meets a zero of psi on the ket side and is never read on the bra side (the walk stays on S),
// and <psi|P|psi> of a term with an odd number of Y is zero, its contribution to O psi imaginary — orthogonal, in the real inner
// product the gradient takes, to every real tangent.  So there is no exactness gate here, as there is for <H^2> (sv_spread_host.hpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "sv_cover_host.hpp"
#include "sv_sparse_layout.hpp"

namespace ovqe {
namespace constrain {

constexpr int OBS_MAX = 8;                       // observables a handle holds
constexpr size_t ENTRY_CAP = (size_t)16 << 20;   // entries of one restricted sum (build_sparse_program's cap)

// support[k], k < m: the basis state of index k (~0ull: a padding slot, skipped); index_of(a): the index of basis state a, or -1 when it
// is outside the support.  Appends to *out; false: more than `cap` entries (out is left with what was built).
template <class IndexOf>
bool restrict_to_support(const std::vector<HGroup> &groups, const std::vector<HTerm> &terms, const uint64_t *support, int m, IndexOf index_of,
                         size_t cap, std::vector<SpEntry> *out) {
    const size_t before = out->size();
    for (const HGroup &g : groups) {
        const uint64_t x = g.x;
        const uint64_t pbit = x ? 1ull << (63 - __builtin_clzll(x)) : 0;
        for (int k = 0; k < m; ++k) {
            const uint64_t a = support[k];
            if (a == ~0ull) continue;
            if (x && (a & pbit)) continue;
            const uint64_t b = a ^ x;
            int kb = k;
            if (x) {
                kb = index_of(b);
                if (kb < 0) continue;
            }
            double d = 0.0;
            for (int t = g.t0; t < g.t1; ++t) {
                const HTerm &ht = terms[t];
                if (__builtin_popcountll(x & ht.z) & 1) continue;  // odd #Y: zero on a real state
                d += (__builtin_popcountll(b & ht.z) & 1) ? -ht.cr : ht.cr;
            }
            if (d == 0.0) continue;
            SpEntry e;
            e.ij = (uint32_t)k | ((uint32_t)kb << 12);
            e.pad = 0;
            e.c = x ? 2.0 * d : d;
            out->push_back(e);
            if (out->size() - before > cap) return false;
        }
    }
    return true;
}

}  // namespace constrain
}  // namespace ovqe
