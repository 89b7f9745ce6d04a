// sv_cover_host.hpp — what every planner of the tiled Pauli-sum paths shares: the table records the tile kernels read, the constants
// that tie planners and kernels together, and the cover rule itself.  Host-only: no HIP, no handle types — g++ compiles it alone
// (tests/cpu/cross_cover_check.cpp and tests/cpu/pool_cover_check.cpp replay the tables built from it the way the kernels index them).
//
// A tile is the set of amplitudes whose index agrees outside a set S of M index bits; an x-group (all terms of one x mask) is evaluated
// from the LDS copy of a tile when its x mask lies inside S.  grow_tile_set() is the one greedy rule that chooses S; its callers are
// build_ham_tiles (tile_host.inc: <H> / sigma on one register), make_plan (sector_host.inc: the <H> sweeps of the sector path),
// cross::build_cover (sv_cross_host.hpp: ovqe_xsum_*) and pool::build_cover (sv_pool_host.hpp: ovqe_xpool_*).  The last two cover the
// groups of one rank difference over chunks of 2^m amplitudes and share the rest as well: pick_pass(), the staged chunks, the
// streaming form by classes of x bits above the chunk.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <map>
#include <set>
#include <tuple>
#include <utility>
#include <vector>

namespace ovqe {

constexpr int TILE_TERM_CAP = 512;      // terms of one staged chunk
constexpr int TILE_APPLY_GROUPS = 128;  // x-groups (pieces) of a chunk staged in LDS (operator-application form)
constexpr int TILE_EXPECT_LOG_NT = 9;   // threads per workgroup of the tile kernels (256 measured faster than 1024): thread / trip masks
// lowest index bits forced into every tile (a real amplitude is 8 bytes: at least one, for 16-byte chunks): fewer forced bits = fewer
// sweeps per H psi / <H> (N2/cc-pVDZ at 24 qubits: 102 sweeps at 4; 25.4 ms per H psi at 2, 30.1 at 4)
constexpr int HAM_TILE_LOW = 2;
// tile bits: complex / real amplitudes (a real tile holds twice the amplitudes in the same 64 KB); chunks below 2^MIN stream
constexpr int TILE_MIN_COMPLEX = 10, TILE_MIN_REAL = 11, TILE_MAX_COMPLEX = 12, TILE_MAX_REAL = 13;

// Hamiltonian / pool term with i^{ny} folded into the coefficient
struct HTerm {
    uint64_t z;
    double cr, ci;
};
struct HGroup {
    uint64_t x;      // local part of the x mask
    uint64_t jbase;  // high (global) bits of the partner's global index
    int32_t t0, t1;  // term range
    double tiny;     // 64 eps sum_t |c_t|: a D_g(j) at or below it is a rounding residue of a sum that cancels (see group_coeff_snap)
};
struct TilePass {    // one pass of a cross-shard cover (k_tile_cross*, k_tile_pool*)
    uint64_t smask, mask_lo, mask_hi;   // tile bits (inside the chunk), thread bits, trip bits (real flavour: in the index space of amplitude PAIRS)
    uint64_t d_out;                     // x bits of the pass's groups outside the tile: other tile = ket tile ^ d_out (local index space)
    int32_t a0, a1;                     // staged chunks of the pass
};
struct ExChunkT {
    int32_t g0, g1, t0, t1;  // entries, terms
};
struct ExAGroupT {    // x-group of the sweep with its raw terms (k_tile_apply)
    uint32_t x;       // tile-local x mask
    int32_t t0, t1;   // terms (absolute, in the apply term table)
    int32_t pad;      // bit 0: every folded coefficient of the piece is real
};
struct ExTermT {
    uint64_t zout;    // z outside the tile
    uint32_t zin;     // z on the tile bits, x positions cleared
    uint32_t pad;
    double cr, ci;    // i^ny and the pattern's sign folded
};
static_assert(sizeof(HTerm) == 24 && sizeof(HGroup) == 32, "records the kernels read");
static_assert(sizeof(TilePass) == 40 && sizeof(ExChunkT) == 16 && sizeof(ExAGroupT) == 16 && sizeof(ExTermT) == 32, "records the kernels read");

inline void fold_iny(double a, double b, int ny, double &cr, double &ci) {   // (a + ib) * i^ny
    switch (ny & 3) {
    case 0: cr = a; ci = b; break;
    case 1: cr = -b; ci = a; break;
    case 2: cr = -a; ci = -b; break;
    default: cr = b; ci = -a; break;
    }
}

inline uint32_t extract_bits(uint64_t v, uint64_t mask) {  // pext
    uint32_t r = 0;
    int k = 0;
    for (uint64_t mk = mask; mk; mk &= mk - 1ull, ++k)
        if ((v >> __builtin_ctzll(mk)) & 1ull) r |= 1u << k;
    return r;
}

inline ExTermT tile_term(const HTerm &t, uint64_t S) {   // a term as the kernels of a tile with bit set S read it
    ExTermT et = {};
    et.zin = extract_bits(t.z, S);
    et.zout = t.z & ~S;
    et.cr = t.cr;
    et.ci = t.ci;
    return et;
}

// The cover rule: a set starts from the seed bits and grows, up to M bits out of the lowest n_bits, by the bit that brings the most
// masks within reach (masks that are nearly inside count more; equal scores: the lowest bit), until no mask that still fits is
// outside; then it is filled up with the lowest free bits.  `masks`: the x masks still to be covered (bits below n_bits only).
inline uint64_t grow_tile_set(const std::vector<uint64_t> &masks, uint64_t seed, int M, int n_bits) {
    static const double wgt[8] = {1.0, 0.25, 0.0625, 0.015625, 0.00390625, 0.0009765625, 0.000244140625, 0.00006103515625};
    uint64_t S = seed;
    while (__builtin_popcountll(S) < M) {
        const int room = M - __builtin_popcountll(S);
        double score[64] = {0.0};
        bool any = false;
        for (const uint64_t x : masks) {
            const uint64_t miss = x & ~S;
            const int nm = __builtin_popcountll(miss);
            if (nm == 0 || nm > room) continue;
            any = true;
            for (uint64_t mk = miss; mk; mk &= mk - 1ull) score[__builtin_ctzll(mk)] += wgt[std::min(nm - 1, 7)];
        }
        if (!any) break;
        int best = -1;
        for (int b = 0; b < n_bits; ++b)
            if (!((S >> b) & 1ull) && (best < 0 || score[b] > score[best])) best = b;
        S |= 1ull << best;
    }
    for (int b = 0; __builtin_popcountll(S) < M; ++b) S |= 1ull << b;
    return S;
}

// the lowest log_nt bits of smask are walked by the threads of a workgroup, the others by its trips -> (mask_lo, mask_hi)
inline std::pair<uint64_t, uint64_t> thread_trip_masks(uint64_t smask, int log_nt) {
    uint64_t lo = 0, mk = smask;
    for (int k = 0; k < log_nt && mk; ++k) {
        lo |= mk & (0ull - mk);
        mk &= mk - 1ull;
    }
    return {lo, smask & ~lo};
}

// ---- staged chunks: the pieces of a pass are staged in LDS chunk by chunk; `open` is the chunk being filled ----
inline ExChunkT open_chunk(size_t n_groups, size_t n_terms) {
    return {(int32_t)n_groups, (int32_t)n_groups, (int32_t)n_terms, (int32_t)n_terms};
}
inline void close_chunk(std::vector<ExChunkT> &chunks, ExChunkT &open, size_t n_groups, size_t n_terms) {
    open.g1 = (int32_t)n_groups;
    open.t1 = (int32_t)n_terms;
    if (open.g1 > open.g0) chunks.push_back(open);
    open = open_chunk(n_groups, n_terms);
}
// before a piece of `add` terms is appended to tables that hold n_groups pieces and n_terms terms: close `open` if the piece would
// take it past a cap
inline void stage_piece(std::vector<ExChunkT> &chunks, ExChunkT &open, size_t n_groups, size_t n_terms, size_t add, int term_cap,
                        int group_cap = INT_MAX) {
    if ((int)n_terms - open.t0 + (int)add > term_cap || (int)n_groups - open.g0 >= group_cap) close_chunk(chunks, open, n_groups, n_terms);
}

// ---- covers of the groups of one rank difference over chunks of 2^m amplitudes (cross-shard sums, pool screen) ----
inline int chunk_tile_bits(int m, bool real) {   // 0: the chunk is too small to tile (streaming form)
    return m < (real ? TILE_MIN_REAL : TILE_MIN_COMPLEX) ? 0 : std::min(real ? TILE_MAX_REAL : TILE_MAX_COMPLEX, m);
}

// The next pass, from the x masks (local index space) that no pass holds yet: the class of x bits above the chunk with the most
// distinct masks left fixes the part of d_out above the chunk (the first such class at equal counts); S grows over the chunk bits
// from the masks of that class; the displacement below the chunk bits is the most frequent leftover (ascending: 0 wins a tie —
// nothing is left over whenever a mask fits S).  The pass takes every item with (x & ~S) == d_out: at least one.
struct PassPick {
    uint64_t S;     // tile bits in the index space of the amplitudes (TilePass::smask is S >> 1 in the real flavour)
    TilePass ps;    // a0 / a1 left to the caller
};
inline PassPick pick_pass(const std::vector<uint64_t> &x_left, int m, int M, bool real) {
    const uint64_t lowmask = (1ull << m) - 1ull;
    std::map<uint64_t, std::set<uint64_t>> left;   // class -> distinct x
    for (const uint64_t x : x_left) left[x >> m].insert(x);
    uint64_t hb = 0;
    size_t best_n = 0;
    for (const auto &kv : left)
        if (kv.second.size() > best_n) hb = kv.first, best_n = kv.second.size();
    std::vector<uint64_t> masks;
    for (const uint64_t x : left[hb]) masks.push_back(x & lowmask);
    PassPick pk = {};
    pk.S = grow_tile_set(masks, (1ull << std::min(HAM_TILE_LOW, M)) - 1ull, M, m);
    std::map<uint64_t, int> leftovers;
    for (const uint64_t x : masks) ++leftovers[x & ~pk.S];
    uint64_t dl = 0;
    int dl_n = -1;
    for (const auto &kv : leftovers)
        if (kv.second > dl_n) dl = kv.first, dl_n = kv.second;
    pk.ps.smask = real ? pk.S >> 1 : pk.S;   // (index bit 0 = the pair bit is always inside a real tile)
    std::tie(pk.ps.mask_lo, pk.ps.mask_hi) = thread_trip_masks(pk.ps.smask, TILE_EXPECT_LOG_NT);
    pk.ps.d_out = (hb << m) | dl;
    return pk;
}

// streaming form (chunks too small to tile): one launch per class of equal x bits above the chunk.  -> the items in ascending class
// order, their order inside a class kept; class_extend() then records the table range [begin, end) an item was given
template <class Item>
std::vector<int> class_order(const std::vector<Item> &items, int m) {
    std::vector<int> order(items.size());
    for (size_t k = 0; k < order.size(); ++k) order[k] = (int)k;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return (items[a].x >> m) < (items[b].x >> m); });
    return order;
}
inline void class_extend(std::vector<uint64_t> &class_h, std::vector<std::pair<int, int>> &ranges, uint64_t hb, size_t begin, size_t end) {
    if (class_h.empty() || class_h.back() != hb) {
        class_h.push_back(hb);
        ranges.push_back({(int)begin, (int)begin});
    }
    ranges.back().second = (int)end;
}

}  // namespace ovqe
