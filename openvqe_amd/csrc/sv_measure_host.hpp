// sv_measure_host.hpp — host-side plan of finite-shot measurement (kernels: sv_measure.hpp; handle section: measure_host.inc; entry
// points ovqe_sample / ovqe_measure_paulis / ovqe_measure_groups / ovqe_energy_sampled / ovqe_measure_info: abi_measure.inc).
// Host-only: no HIP, no handle types — g++ compiles it alone (tests/cpu/measure_plan_check.cpp checks the grouping against its rule).
//
// MEASUREMENT GROUPS.  A Pauli string acts on qubit (index bit) b with the letter X if x & ~z, Y if x & z, Z if z & ~x.  A group is a
// set of strings that agree letter by letter wherever two of them act (qubit-wise commutation); its basis — X on the bits of xbasis, Y
// on those of ybasis, Z elsewhere — diagonalises all of them at once, and one shot of the group gives every term's eigenvalue:
// (-1)^popcount(outcome & (x | z)).  The rule (include/ovqe_sv.h restates it):
//   identity terms go to the constant (group -1); the others are taken by |coeff| descending, ties by stored position; each goes into
//   the FIRST group whose basis agrees with it on every bit where both act, and extends that group's basis; groups are numbered in
//   creation order.
//
// BASIS CHANGE.  phi = B psi, B = (x) over the bits of (H on xbasis, H S^+ on ybasis).  The bits below the LDS tile are rotated inside
// the copy of psi (one launch), every bit above it takes one streaming pass over phi.
//
// SCAN.  The inclusive prefix sums of p = |phi|^2 in index order: chunks of SCAN_CHUNK elements scanned by one workgroup each, the chunk
// totals scanned by ONE workgroup that walks them 256 at a time with a carry (one stage at every register size: 2^22 totals at 33
// qubits are 16384 steps of that workgroup), then the offsets added.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

namespace ovqe {
namespace measure {

constexpr int TILE_BITS = 11;                    // amplitudes of one LDS tile of the basis change: 2^11 x 16 B = 32 KiB
constexpr int SCAN_THREADS = 256, SCAN_PER_THREAD = 8;
constexpr int SCAN_CHUNK = SCAN_THREADS * SCAN_PER_THREAD;   // elements per workgroup of the chunk scan
constexpr int DRAW_THREADS = 256;                // one lane per shot

struct Plan {
    std::vector<int32_t> group_of_term;          // per stored term: its group, -1 for identity terms
    std::vector<uint64_t> xbasis, ybasis, zbasis;   // per group: bits measured in X / Y, and bits some term reads in Z
    std::vector<int64_t> first;                  // per group: its terms are members[first[g] .. first[g + 1])
    std::vector<int32_t> members;                // stored positions, in the order they joined
    double constant = 0.0;                       // sum of the identity terms' coefficients
    int groups() const { return (int)xbasis.size(); }
};

inline Plan plan_groups(int64_t T, const uint64_t *x, const uint64_t *z, const double *coeff) {
    Plan P;
    P.group_of_term.assign((size_t)T, -1);
    std::vector<int32_t> order;
    for (int64_t t = 0; t < T; ++t) {
        if ((x[t] | z[t]) == 0) P.constant += coeff[t];
        else order.push_back((int32_t)t);
    }
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return std::fabs(coeff[a]) > std::fabs(coeff[b]); });
    std::vector<std::vector<int32_t>> lists;
    for (int32_t t : order) {
        const uint64_t tx = x[t] & ~z[t], ty = x[t] & z[t], tz = z[t] & ~x[t];
        int g = 0;
        for (; g < P.groups(); ++g)
            if (!((tx & (P.ybasis[g] | P.zbasis[g])) | (ty & (P.xbasis[g] | P.zbasis[g])) | (tz & (P.xbasis[g] | P.ybasis[g])))) break;
        if (g == P.groups()) {
            P.xbasis.push_back(0);
            P.ybasis.push_back(0);
            P.zbasis.push_back(0);
            lists.emplace_back();
        }
        P.xbasis[g] |= tx;
        P.ybasis[g] |= ty;
        P.zbasis[g] |= tz;
        P.group_of_term[t] = g;
        lists[g].push_back(t);
    }
    P.first.push_back(0);
    for (const std::vector<int32_t> &l : lists) {
        P.members.insert(P.members.end(), l.begin(), l.end());
        P.first.push_back((int64_t)P.members.size());
    }
    return P;
}

// the basis masks of a measurement are disjoint and inside the register
inline bool basis_ok(int n, uint64_t xbasis, uint64_t ybasis) {
    const uint64_t all = n >= 64 ? ~0ull : (1ull << n) - 1ull;
    return !(xbasis & ybasis) && !((xbasis | ybasis) & ~all);
}

struct Geometry {
    int tile_bits;          // min(n, TILE_BITS)
    uint64_t tiles;         // workgroups of the fused copy + in-tile butterflies
    uint64_t low_x, low_y;  // rotated bits inside the tile
    std::vector<int> high;  // rotated bits above it, ascending: one streaming pass each
    std::vector<int> high_y;   // ... 1 where the bit is measured in Y
    uint64_t chunks;        // workgroups of the chunk scan = entries of the totals array
    size_t prefix_bytes, phi_bytes, totals_bytes;   // phi is needed only when `high` is not empty
};

inline Geometry geometry(int n, uint64_t xbasis, uint64_t ybasis) {
    Geometry G;
    const uint64_t N = 1ull << n;
    G.tile_bits = std::min(n, TILE_BITS);
    G.tiles = N >> G.tile_bits;
    const uint64_t low = (1ull << G.tile_bits) - 1ull;
    G.low_x = xbasis & low;
    G.low_y = ybasis & low;
    for (int b = G.tile_bits; b < n; ++b)
        if (((xbasis | ybasis) >> b) & 1ull) {
            G.high.push_back(b);
            G.high_y.push_back((int)((ybasis >> b) & 1ull));
        }
    G.chunks = (N + SCAN_CHUNK - 1) / SCAN_CHUNK;
    G.prefix_bytes = (size_t)N * sizeof(double);
    G.phi_bytes = (size_t)N * 2 * sizeof(double);
    G.totals_bytes = (size_t)G.chunks * sizeof(double);
    return G;
}

// energy = constant + sum_g mean_g, std_error = sqrt(sum_g s_g^2 / n_shots) with s_g^2 the unbiased sample variance of group g, from
// the groups' (sum v, sum v^2).  A variance that rounding leaves below zero counts as zero.
inline void estimate(double constant, int64_t n_shots, const std::vector<double> &sum_v, const std::vector<double> &sum_v2, double *energy,
                     double *std_error) {
    const double n = (double)n_shots;
    double e = constant, var = 0.0;
    for (size_t g = 0; g < sum_v.size(); ++g) {
        e += sum_v[g] / n;
        const double s2 = (sum_v2[g] - sum_v[g] * sum_v[g] / n) / (n - 1.0);
        var += std::max(s2, 0.0);
    }
    *energy = e;
    *std_error = std::sqrt(var / n);
}

}  // namespace measure
}  // namespace ovqe
