// sv_cross_host.hpp — host-side planner of the Pauli sums ACROSS two shards of the partitioned register (kernels: sv_cross.hpp; entry
// points ovqe_xsum_*: cross_host.inc).  Host-only: no HIP, no handle types — g++ compiles it alone (tests/cpu/cross_cover_check.cpp
// replays its tables the way the kernels index them).
//
// The x-groups of one rank difference d (local x masks; the partner's shard arrives in chunks of 2^m amplitudes — sigma = H psi on
// real amplitudes takes the d = 0 groups the same way, the shard being its one chunk, m = n_local) are covered by passes (tile bit
// set S inside the chunk, displacement d_out outside it) chosen by pick_pass() of sv_cover_host.hpp; a pass holds every group with
// (x & ~S) == d_out in the operator-application form of the tile kernels (staged chunks of pieces and terms).  Chunks too small to
// tile keep the groups as they are, in classes of equal x bits above the chunk (k_cross_small).
#pragma once
#include "sv_cover_host.hpp"

namespace ovqe {
namespace cross {

struct RawGroup {
    uint64_t x;                 // local x mask
    std::vector<HTerm> terms;   // full z masks, i^ny folded
};

struct Cover {                  // the groups of one partner (rank difference d) in one flavour
    uint64_t d = 0;
    int ngroups = 0, nterms = 0;
    bool small = false;         // chunks below the tile sizes: k_cross_small, one launch per class of high x bits
    int M = 0;                  // tile bits of the passes
    std::vector<TilePass> passes;
    std::vector<ExChunkT> achunks;   // tile form
    std::vector<ExAGroupT> agroups;
    std::vector<ExTermT> aterms;
    std::vector<uint64_t> class_h;                   // small form: x bits above the chunk per class ...
    std::vector<std::pair<int, int>> class_groups;   // ... and its group range
    std::vector<HGroup> groups;
    std::vector<HTerm> terms;
    int64_t n_passes() const { return small ? (int64_t)class_h.size() : (int64_t)passes.size(); }
};

// cover of one partner's groups for chunks of 2^m amplitudes.  drop_imaginary: between real vectors a term with an imaginary folded
// coefficient (odd number of Y) contributes nothing to <H> or to a real sigma and is left out.  -> false: a pass took no group
inline bool build_cover(Cover &C, std::vector<RawGroup> groups, int m, bool real, bool drop_imaginary) {
    if (drop_imaginary) {
        for (RawGroup &g : groups)
            g.terms.erase(std::remove_if(g.terms.begin(), g.terms.end(), [](const HTerm &t) { return t.ci != 0.0; }), g.terms.end());
        groups.erase(std::remove_if(groups.begin(), groups.end(), [](const RawGroup &g) { return g.terms.empty(); }), groups.end());
    }
    const int G = (int)groups.size();
    C.ngroups = G;
    C.nterms = 0;
    for (const RawGroup &g : groups) C.nterms += (int)g.terms.size();
    C.M = chunk_tile_bits(m, real);
    if (!C.M) {   // too small to tile: classes of equal high x bits, one streaming launch each
        C.small = true;
        for (int g : class_order(groups, m)) {
            HGroup gr = {};
            gr.x = groups[g].x & ((1ull << m) - 1ull);
            gr.t0 = (int32_t)C.terms.size();
            C.terms.insert(C.terms.end(), groups[g].terms.begin(), groups[g].terms.end());
            gr.t1 = (int32_t)C.terms.size();
            class_extend(C.class_h, C.class_groups, groups[g].x >> m, C.groups.size(), C.groups.size() + 1);
            C.groups.push_back(gr);
        }
        return true;
    }
    std::vector<char> done(G, 0);
    int remaining = G;
    while (remaining > 0) {
        std::vector<uint64_t> x_left;
        for (int g = 0; g < G; ++g)
            if (!done[g]) x_left.push_back(groups[g].x);
        PassPick pk = pick_pass(x_left, m, C.M, real);
        pk.ps.a0 = (int32_t)C.achunks.size();
        ExChunkT open = open_chunk(C.agroups.size(), C.aterms.size());
        int took = 0;
        for (int g = 0; g < G; ++g) {
            if (done[g] || (groups[g].x & ~pk.S) != pk.ps.d_out) continue;
            done[g] = 1;
            --remaining;
            ++took;
            const uint32_t xl = extract_bits(groups[g].x, pk.S);
            const std::vector<HTerm> &ts = groups[g].terms;
            for (size_t k0 = 0; k0 < ts.size(); k0 += TILE_TERM_CAP) {   // (oversized groups in pieces: D_g is a sum over the terms)
                const size_t k1 = std::min(ts.size(), k0 + (size_t)TILE_TERM_CAP);
                stage_piece(C.achunks, open, C.agroups.size(), C.aterms.size(), k1 - k0, TILE_TERM_CAP, TILE_APPLY_GROUPS);
                ExAGroupT ag = {xl, (int32_t)C.aterms.size(), 0, 1};
                for (size_t k = k0; k < k1; ++k) {
                    C.aterms.push_back(tile_term(ts[k], pk.S));
                    if (ts[k].ci != 0.0) ag.pad = 0;   // bit 0 of pad: every folded coefficient of the piece is real
                }
                ag.t1 = (int32_t)C.aterms.size();
                C.agroups.push_back(ag);
            }
        }
        close_chunk(C.achunks, open, C.agroups.size(), C.aterms.size());
        pk.ps.a1 = (int32_t)C.achunks.size();
        if (took == 0) return false;
        C.passes.push_back(pk.ps);
    }
    return true;
}

}  // namespace cross
}  // namespace ovqe
