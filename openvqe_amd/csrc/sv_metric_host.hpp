// sv_metric_host.hpp — host-side plan of the Fubini-Study metric of the ansatz state (kernels: k_sparse_metric in sv_sparse.hpp and
// sv_metric.hpp; handle section: metric_host.inc; entry points ovqe_metric_tensor / ovqe_metric_info: abi_metric.inc).  Host-only: no
// HIP, no handle types — g++ compiles it alone (tests/cpu/metric_plan_check.cpp replays its tables the way the kernels index them and
// compares with a dense simulation).
//
//   T_k = d psi / d theta_k,   g_ij = Re( <T_i|T_j> - <T_i|psi><psi|T_j> ),   psi = U(theta)|hf>
//
// COMPACT SUPPORT (path 1).  A real program (every rotation string with an odd number of Y) moves amplitudes between the two members
// of pairs (i, i ^ x) only, by a Givens rotation: with i0 the member whose pivot bit (highest bit of x) is clear, u = a[i0], v = a[i0 ^ x],
//   u' = c u + sigma s v,   v' = c v - sigma s u,   (c, s) = cos / sin of the entry's angle, sigma = +-1 the pair's sign.
// The support reachable from |hf> is propagated through the fused-kernel program — OP_TAB runs with their host-computed pattern
// constants, plain same-x runs rotation by rotation — and the program is restated on compact indices: per op a list of pair words and
// one table entry (coeff, phi0, parameter) per distinct angle.  Unlike the energy kernels' compact program this one needs no
// Hamiltonian and keeps constant angles (pidx < 0) and offsets (phi0), which are part of the metric's contract.
#pragma once
#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "sv_rdm_host.hpp"
#include "sv_sparse_layout.hpp"

namespace ovqe {
namespace metric {

constexpr int KIND_ROT = 0, KIND_TAB = 5;   // SmallOpKind OP_PAIR / OP_TAB (sv_small.hpp)
constexpr int MAX_SUPPORT = 4096;           // 12-bit compact indices
constexpr int MAX_PATTERNS = 127;           // 7-bit pattern field of a pair word

struct InOp {     // one op of the fused-kernel program
    uint64_t x, zc;   // pair mask; KIND_TAB: the run's z mask outside x
    int kind, first, count;
};
struct InRot {    // its table entries (KIND_TAB: z = the pattern's bits on the x positions)
    uint64_t z;
    double coeff, phi0;
    int32_t pidx, ny;
};

struct TabEntry {   // angle of the entry: coeff * theta[pidx] + phi0 (pidx < 0: phi0 alone)
    double coeff, phi0;
    int32_t pidx, pad;
};
using Op = SpOp;     // the op record and the pair word of the compact kernels (sv_sparse_layout.hpp); ci: the member with the pivot bit clear

struct Compact {
    int m = 0, hf = 0;               // support size, compact index of |hf>
    std::vector<Op> ops;
    std::vector<uint32_t> pairs;
    std::vector<TabEntry> tab;
    std::vector<int32_t> first_op;   // [K]: the first op with a table entry of parameter k (ops.size(): none — a zero tangent)
    std::vector<uint64_t> support;   // [m]: the basis state behind every compact index (sv_hessian_host.hpp restricts the Hamiltonian to it)
};

inline int parity64(uint64_t v) { return __builtin_popcountll(v) & 1; }

// false: the program has no compact real form (a diagonal or even-Y rotation, a literal gate, a support beyond MAX_SUPPORT)
inline bool build_compact(uint64_t hf, const std::vector<InOp> &ops, const std::vector<InRot> &rots, int K, Compact *out) {
    Compact &C = *out;
    C = Compact();
    std::unordered_map<uint64_t, int> id;
    std::vector<uint64_t> S;
    auto get = [&](uint64_t a) {
        auto it = id.find(a);
        if (it != id.end()) return it->second;
        const int k = (int)S.size();
        id.emplace(a, k);
        S.push_back(a);
        return k;
    };
    get(hf);
    std::unordered_set<uint64_t> seen;
    for (const InOp &op : ops) {
        if ((op.kind != KIND_ROT && op.kind != KIND_TAB) || op.x == 0 || op.count < 0) return false;
        if ((size_t)op.first + (size_t)op.count > rots.size()) return false;
        const uint64_t x = op.x, pbit = 1ull << (63 - __builtin_clzll(x));
        if (op.kind == KIND_TAB) {
            if (op.count > MAX_PATTERNS) return false;
            Op so{(int32_t)C.pairs.size(), 0, (int32_t)C.tab.size(), 0};
            for (int p = 0; p < op.count; ++p) {
                const InRot &r = rots[(size_t)op.first + p];
                if (r.phi0 != 0.0 || r.pidx < 0) return false;
                C.tab.push_back(TabEntry{r.coeff, 0.0, r.pidx, 0});
            }
            seen.clear();
            const size_t s0 = S.size();
            for (size_t k = 0; k < s0; ++k) {
                const uint64_t a = S[k], i0 = (a & pbit) ? (a ^ x) : a;
                if (!seen.insert(i0).second) continue;
                for (int p = 0; p < op.count; ++p) {
                    if ((i0 & x) != rots[(size_t)op.first + p].z) continue;
                    const int ci = get(i0), cj = get(i0 ^ x);
                    if ((int)S.size() > MAX_SUPPORT) return false;
                    C.pairs.push_back((uint32_t)ci | ((uint32_t)cj << 12) | ((uint32_t)parity64(i0 & op.zc) << 24) | ((uint32_t)p << 25));
                    break;
                }
            }
            so.npairs = (int32_t)C.pairs.size() - so.first;
            if (so.npairs > 0) C.ops.push_back(so);
            else C.tab.resize((size_t)so.tab0);
            continue;
        }
        // a plain run: one op per rotation.  exp(-i phi P) with an odd number ny of Y acts on the pair as the Givens rotation above with
        // sigma s = -eta (-1)^{parity(i0 & z)} sin(phi), eta = +1 (ny = 1), -1 (ny = 3): the entry holds -eta (coeff, phi0), the word the parity
        for (int q = 0; q < op.count; ++q) {
            const InRot &r = rots[(size_t)op.first + q];
            if (!(r.ny & 1)) return false;
            const double f = (r.ny & 2) ? 1.0 : -1.0;
            Op so{(int32_t)C.pairs.size(), 0, (int32_t)C.tab.size(), 0};
            C.tab.push_back(TabEntry{f * r.coeff, f * r.phi0, r.pidx, 0});
            seen.clear();
            const size_t s0 = S.size();
            for (size_t k = 0; k < s0; ++k) {
                const uint64_t a = S[k], i0 = (a & pbit) ? (a ^ x) : a;
                if (!seen.insert(i0).second) continue;
                const int ci = get(i0), cj = get(i0 ^ x);
                if ((int)S.size() > MAX_SUPPORT) return false;
                C.pairs.push_back((uint32_t)ci | ((uint32_t)cj << 12) | ((uint32_t)parity64(i0 & r.z) << 24));
            }
            so.npairs = (int32_t)C.pairs.size() - so.first;
            C.ops.push_back(so);
        }
    }
    C.m = (int)S.size();
    C.hf = 0;
    C.support = S;
    C.first_op.assign((size_t)std::max(K, 0), (int32_t)C.ops.size());
    for (int o = (int)C.ops.size() - 1; o >= 0; --o) {
        const int ntab = (o + 1 < (int)C.ops.size() ? C.ops[(size_t)o + 1].tab0 : (int)C.tab.size()) - C.ops[(size_t)o].tab0;
        for (int e = 0; e < ntab; ++e) {
            const int32_t p = C.tab[(size_t)C.ops[(size_t)o].tab0 + e].pidx;
            if (p >= 0 && p < K) C.first_op[(size_t)p] = o;
        }
    }
    return true;
}

// ---- the tangent store: INDEX-MAJOR, row = amplitude (compact index, or register index on the streaming path), column = vector,
// padded to the Gram block, so that the Gram kernel of the density matrices (k_rdm_gram, sv_rdm.hpp) reads it as it stands.
//   compact support: doubles, column k = T_k                       (<psi|T_k> = 0 on a real state: g is the Gram matrix itself)
//   streaming:       16-byte amplitudes, column 0 = psi, 1 + k = T_k  (the Gram matrix's first column is <T_k|psi>)
struct Store {
    int64_t rows = 0, width = 0, wpad = 0;
    size_t elem_bytes = 0, bytes = 0;
};
inline Store store_layout(int64_t rows, int64_t K, bool compact) {
    Store s;
    s.rows = rows;
    s.width = compact ? K : K + 1;
    s.wpad = (s.width + rdm::GRAM_BLOCK - 1) / rdm::GRAM_BLOCK * rdm::GRAM_BLOCK;
    s.elem_bytes = compact ? 8 : 16;
    s.bytes = (size_t)rows * (size_t)s.wpad * s.elem_bytes;
    return s;
}

// the Gram kernel's schedule over the whole store as ONE chunk: block pairs (upper triangle) x row slices, four workgroups per CU
inline rdm::Schedule gram_plan(const Store &st, int num_cus) {
    rdm::Schedule s;
    s.real = st.elem_bytes == 8;
    s.width = st.width;
    s.wpad = st.wpad;
    s.nblk = (int)(st.wpad / rdm::GRAM_BLOCK);
    s.npairs = s.nblk * (s.nblk + 1) / 2;
    s.elem_bytes = st.elem_bytes;
    s.row_bytes = (size_t)st.wpad * st.elem_bytes;
    s.tile_rows = (int)(rdm::GRAM_TILE_BYTES / (rdm::GRAM_BLOCK * st.elem_bytes));
    s.rows = st.rows;
    s.chunk_rows = std::max<int64_t>(1, (st.rows + s.tile_rows - 1) / s.tile_rows) * s.tile_rows;
    s.nchunks = 1;
    const int64_t tiles = s.chunk_rows / s.tile_rows;
    const int64_t want = ((int64_t)4 * std::max(num_cus, 1) + s.npairs - 1) / std::max(s.npairs, 1);
    s.slices = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, tiles), rdm::GRAM_MAX_SLICES));
    s.slice_rows = (tiles + s.slices - 1) / s.slices * s.tile_rows;
    s.slices = (int)((s.chunk_rows + s.slice_rows - 1) / s.slice_rows);
    s.workspace_bytes = st.bytes;
    s.slab_elems = (size_t)s.npairs * s.slices * rdm::GRAM_BLOCK * rdm::GRAM_BLOCK;
    return s;
}

}  // namespace metric
}  // namespace ovqe
