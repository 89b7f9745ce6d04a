// sv_pool_host.hpp — host-side planner of the ADAPT pool screen on one shard of the index-bit-partitioned register (kernels:
// sv_pool.hpp; entry points ovqe_xpool_*: pool_host.inc; protocol: openvqe_amd/distributed.py pool_gradients).  Host-only: no HIP,
// no handle types — g++ compiles it alone (tests/cpu/pool_cover_check.cpp replays its tables the way the kernels index them).
//
// v_k = sum_t c_t <sigma| P_t |psi> over the terms of pool operator k (ref:openvqe/adapt/fermionic_adapt_vqe.py:67-73,
// ref:openvqe/adapt/qubit_adapt_vqe.py:147-150).  Masks arrive in the PHYSICAL index-bit space of the whole register.  A term's x
// part on the rank bits, d = x >> n_local, names the partner shard its ket amplitudes live in; that shard arrives in chunks of 2^m
// amplitudes (d = 0: the shard itself is its one chunk, m = n_local).  Per rank difference the work items are ENTRIES — one
// (operator, local x mask) pair with its terms, cut into pieces of at most POOL_TERM_CAP terms that feed the same accumulator — and
// the distinct local x masks are covered by passes (tile bit set S inside the chunk, displacement d_out outside it) chosen by
// pick_pass() of sv_cover_host.hpp, as in the cross-shard sums: S grows by grow_tile_set(); the x bits above the chunk, which pair
// ket chunk c with bra chunk c ^ h, are part of d_out.  Two entries with the same x that belong to different operators never merge.
#pragma once
#include "sv_cover_host.hpp"

#include <string>

namespace ovqe {
namespace pool {

constexpr int POOL_TERM_CAP = 256;    // terms of one staged chunk of a pass
constexpr int POOL_ENTRY_CAP = 64;    // entries (pieces) of one staged chunk
static_assert(POOL_TERM_CAP <= TILE_TERM_CAP && POOL_ENTRY_CAP <= TILE_APPLY_GROUPS, "the pool tables respect the tile caps");
constexpr int POOL_ROWS = 512;        // partial rows: workgroups of a tile pass (grid-stride over the tiles), whatever the shard
constexpr int POOL_SMALL_ROWS = 16;   // ... of the streaming form

struct PoolEntry {
    uint32_t x;        // tile form: tile-local x mask; streaming form: x on the chunk bits
    int32_t t0, t1;    // terms (absolute; ExTermT — streaming form: zout = the full z mask, zin = 0)
    int32_t slot;      // operator k: the accumulator the entry feeds
    int32_t run;       // entries of this chunk from here on that feed the same slot (0: not the first of its run)
    int32_t pad;
};
static_assert(sizeof(PoolEntry) == 24, "record the kernels read");
struct RawEntry {      // one (operator, local x mask) pair of one rank difference
    int32_t slot;
    uint64_t x;
    std::vector<HTerm> terms;   // full z masks, i^ny folded
};

struct Cover {         // the entries of one rank difference in one flavour
    uint64_t d = 0;
    int m = 0;                 // chunk bits
    bool small = false;        // streaming form
    int M = 0;                 // tile bits
    int n_entries = 0, n_x = 0, n_terms = 0;   // (operator, x) pairs, distinct x masks, terms
    std::vector<TilePass> passes;
    std::vector<ExChunkT> chunks;
    std::vector<PoolEntry> entries;
    std::vector<ExTermT> terms;
    std::vector<uint64_t> class_h;                    // streaming form: x bits above the chunk per class ...
    std::vector<std::pair<int, int>> class_entries;   // ... and its entry range
    int64_t n_passes() const { return small ? (int64_t)class_h.size() : (int64_t)passes.size(); }
};

// bytes of the partial sums of a plan: POOL_ROWS rows of one double2 per operator — independent of the shard and of the entries
inline size_t partial_bytes(int64_t n_ops) { return (size_t)POOL_ROWS * (size_t)std::max<int64_t>(n_ops, 1) * 16u; }

// the pool terms by rank difference -> (operator, local x) entries, ascending (d, operator, x): the same plan on every rank.
// -> empty string, or what is wrong with the input
inline std::string collect(int n_local, int n_total, int64_t n_ops, const int64_t *offsets, const uint64_t *x, const uint64_t *z,
                           const double *cre, const double *cim, std::map<uint64_t, std::vector<RawEntry>> &by_d) {
    if (n_ops < 0 || (n_ops && !offsets)) return "operator count / offsets";
    if (n_ops && offsets[0] != 0) return "offsets must start at 0 and never decrease";
    for (int64_t k = 0; k < n_ops; ++k)
        if (offsets[k + 1] < offsets[k]) return "offsets must start at 0 and never decrease";
    const uint64_t allmask = n_total >= 64 ? ~0ull : ((1ull << n_total) - 1ull);
    const uint64_t lmask = (1ull << n_local) - 1ull;
    for (int64_t k = 0; k < n_ops; ++k) {
        std::map<std::pair<uint64_t, uint64_t>, RawEntry> mine;
        for (int64_t t = offsets[k]; t < offsets[k + 1]; ++t) {
            if ((x[t] | z[t]) & ~allmask) return "Pauli mask has bits beyond the register";
            const double a = cre[t], b = cim ? cim[t] : 0.0;
            HTerm rt;
            rt.z = z[t];
            fold_iny(a, b, __builtin_popcountll(x[t] & z[t]), rt.cr, rt.ci);
            RawEntry &e = mine[{x[t] >> n_local, x[t] & lmask}];
            e.slot = (int32_t)k;
            e.x = x[t] & lmask;
            e.terms.push_back(rt);
        }
        for (auto &kv : mine) by_d[kv.first.first].push_back(std::move(kv.second));
    }
    return std::string();
}

// cover of one rank difference's entries for chunks of 2^m amplitudes.  Both flavours keep every term: between real vectors a real
// folded coefficient feeds Re v_k and an imaginary one Im v_k.
inline void build_cover(Cover &C, const std::vector<RawEntry> &raw, int m, bool real) {
    C.m = m;
    C.n_entries = (int)raw.size();
    std::set<uint64_t> xs;
    for (const RawEntry &e : raw) {
        xs.insert(e.x);
        C.n_terms += (int)e.terms.size();
    }
    C.n_x = (int)xs.size();
    // pieces of entry e appended to the tables; tile form (S != 0): `open` is the staged chunk being filled
    auto append = [&](const RawEntry &e, uint32_t xl, uint64_t S, ExChunkT &open) {
        size_t k0 = 0;
        do {
            const size_t k1 = std::min(e.terms.size(), k0 + (size_t)POOL_TERM_CAP);
            if (S) stage_piece(C.chunks, open, C.entries.size(), C.terms.size(), k1 - k0, POOL_TERM_CAP, POOL_ENTRY_CAP);
            PoolEntry pe = {xl, (int32_t)C.terms.size(), 0, e.slot, 0, 0};
            for (size_t k = k0; k < k1; ++k) C.terms.push_back(tile_term(e.terms[k], S));
            pe.t1 = (int32_t)C.terms.size();
            C.entries.push_back(pe);
            k0 = k1;
        } while (k0 < e.terms.size());
    };
    // run heads: within a staged chunk one thread adds the consecutive entries of a slot to that slot's partial
    auto mark_runs = [&](int g0, int g1) {
        for (int g = g0; g < g1;) {
            int r = g + 1;
            while (r < g1 && C.entries[r].slot == C.entries[g].slot) ++r;
            C.entries[g].run = r - g;
            g = r;
        }
    };
    C.M = chunk_tile_bits(m, real);
    if (!C.M) {   // classes of equal high x bits, one streaming launch each
        C.small = true;
        ExChunkT none = {};
        for (int e : class_order(raw, m)) {
            const size_t begin = C.entries.size();
            append(raw[e], (uint32_t)(raw[e].x & ((1ull << m) - 1ull)), 0, none);
            class_extend(C.class_h, C.class_entries, raw[e].x >> m, begin, C.entries.size());
        }
        return;
    }
    const int E = (int)raw.size();
    std::vector<char> done(E, 0);
    int remaining = E;
    while (remaining > 0) {
        std::vector<uint64_t> x_left;
        for (int e = 0; e < E; ++e)
            if (!done[e]) x_left.push_back(raw[e].x);
        PassPick pk = pick_pass(x_left, m, C.M, real);
        pk.ps.a0 = (int32_t)C.chunks.size();
        ExChunkT open = open_chunk(C.entries.size(), C.terms.size());
        for (int e = 0; e < E; ++e) {   // (operator order: the pieces of a slot are consecutive, so runs are as long as they can be)
            if (done[e] || (raw[e].x & ~pk.S) != pk.ps.d_out) continue;
            done[e] = 1;
            --remaining;
            append(raw[e], extract_bits(raw[e].x, pk.S), pk.S, open);
        }
        close_chunk(C.chunks, open, C.entries.size(), C.terms.size());
        pk.ps.a1 = (int32_t)C.chunks.size();
        for (int ch = pk.ps.a0; ch < pk.ps.a1; ++ch) mark_runs(C.chunks[ch].g0, C.chunks[ch].g1);
        C.passes.push_back(pk.ps);   // (the most frequent leftover of a non-empty class always takes at least one entry)
    }
}

}  // namespace pool
}  // namespace ovqe
