// cross_cover_check.cpp — the host-side planner of the cross-shard Pauli sums (openvqe_amd/csrc/sv_cross_host.hpp over
// sv_cover_host.hpp) compiled alone with g++ (ASan + UBSan: tests/test_cross_cover.py).  For random registers (n_local 4..14, 0..3 rank
// bits, chunk bits from 2 up to n_local: the streaming form and tiles of 2^10 .. 2^13 all occur) and random Pauli sums (real-symmetric;
// with odd-Y strings; with complex coefficients; a group of more terms than the term cap; more groups in a pass than the group cap; x
// bits above the chunk and on the rank bits) the cover of every rank difference — d = 0 with the shard as its one chunk, as sigma = H psi
// on real amplitudes takes it — is replayed for every rank the way k_tile_cross / k_tile_cross_real / k_cross_small / k_cross_small_real
// index it: tile base by zero insertion, thread / trip masks, d_out pairing ket chunk c with output chunk c ^ h, signs from zin on the
// ket's tile-local index and from zout on its global index, the pair-index masks of the real flavour.  DOT (<phi|H|psi>) and APPLY
// (H psi) are compared with the term-by-term definition to 1e-12 max(1, |c|_1): the complex flavour on every sum, the real flavour on
// real vectors — DOT and APPLY for real-symmetric sums, DOT for real coefficients with odd-Y strings (their terms are dropped; they
// vanish between real vectors).  Conditions on the tables: every group lies in exactly one pass with all its terms, within a pass ket
// tile -> output tile is a bijection of the shard's tiles (the no-atomics invariant of sv_cross.hpp), staged chunks respect
// TILE_TERM_CAP and TILE_APPLY_GROUPS, passes per partner <= its groups.
//   usage: cross_cover_check <cases> <seed> [hash]      (hash: also print one 64-bit hash over every table built)
#include "../../openvqe_amd/csrc/sv_cross_host.hpp"

#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <random>

using namespace ovqe;
using namespace ovqe::cross;
typedef std::complex<double> cplx;

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                \
            if (++failures > 20) std::exit(1); \
        }                                     \
    } while (0)

static uint64_t table_hash = 1469598103934665603ull;   // FNV-1a over the bytes of every table
static void hash_bytes(const void *p, size_t n) {
    for (size_t k = 0; k < n; ++k) table_hash = (table_hash ^ ((const unsigned char *)p)[k]) * 1099511628211ull;
}
template <class T>
static void hash_vec(const std::vector<T> &v) {   // (every record is free of implicit padding and value-initialised)
    const uint64_t n = v.size();
    hash_bytes(&n, sizeof n);
    if (n) hash_bytes(v.data(), n * sizeof(T));
}
static void hash_cover(const Cover &C) {
    const int64_t head[5] = {(int64_t)C.d, C.ngroups, C.nterms, C.small ? 1 : 0, C.M};
    hash_bytes(head, sizeof head);
    hash_vec(C.passes), hash_vec(C.achunks), hash_vec(C.agroups), hash_vec(C.aterms);
    hash_vec(C.class_h), hash_vec(C.class_groups), hash_vec(C.groups), hash_vec(C.terms);
}

static uint64_t spread(uint64_t v, uint64_t mask) {   // pdep
    uint64_t r = 0;
    for (; mask; mask &= mask - 1ull, v >>= 1)
        if (v & 1ull) r |= mask & (0ull - mask);
    return r;
}
static uint64_t tile_base(uint64_t tl, uint64_t smask) {   // the kernel's insert_zero loop
    for (uint64_t mk = smask; mk; mk &= mk - 1ull) {
        const int p = __builtin_ctzll(mk);
        const uint64_t low = (1ull << p) - 1ull;
        tl = ((tl & ~low) << 1) | (tl & low);
    }
    return tl;
}
static double psign(uint64_t v) { return (__builtin_popcountll(v) & 1) ? -1.0 : 1.0; }

struct Sum {
    std::vector<uint64_t> x, z;
    std::vector<double> cr, ci;
    void term(uint64_t xx, uint64_t zz, double a, double b) { x.push_back(xx), z.push_back(zz), cr.push_back(a), ci.push_back(b); }
};
typedef std::map<uint64_t, std::map<uint64_t, RawGroup>> ByD;   // d -> local x -> group (ascending: the same plan on every rank)

struct Seen {
    int tiled = 0, streamed = 0, multi_pass = 0, cut = 0, multi_chunk = 0, group_cap = 0, above_chunk = 0, dropped = 0, bits[14] = {0};
};

// one rank's share of <phi|H|psi> and of H psi from the plan tables, as the kernels run it
template <bool REAL>
static void replay_rank(int nl, uint64_t rank, const ByD &by_d, int chunk_bits, bool drop, const std::vector<cplx> &psi,
                        const std::vector<cplx> &phi, cplx &dot, std::vector<cplx> &sigma, Seen &seen) {
    const uint64_t shard = 1ull << nl;
    const int NT = 1 << TILE_EXPECT_LOG_NT;
    for (const auto &kv : by_d) {
        const uint64_t d = kv.first;
        const int m = d ? chunk_bits : nl;
        const uint64_t csize = 1ull << m;
        std::vector<RawGroup> groups;
        std::map<uint64_t, int> want;   // x -> terms the tables must hold
        for (const auto &g : kv.second) {
            groups.push_back(g.second);
            int keep = 0;
            for (const HTerm &t : g.second.terms) keep += (drop && t.ci != 0.0) ? 0 : 1;
            if (keep) want[g.first] = keep;
            if (keep != (int)g.second.terms.size()) seen.dropped++;
        }
        Cover C;
        C.d = d;
        CHECK(build_cover(C, groups, m, REAL, drop), "the cover made no progress");
        hash_cover(C);
        // --- conditions on the tables
        CHECK(C.ngroups == (int)want.size(), "group count %d != %zu", C.ngroups, want.size());
        CHECK(C.n_passes() <= (int64_t)want.size(), "passes %lld > groups %zu", (long long)C.n_passes(), want.size());
        CHECK(C.small == (m < (REAL ? 11 : 10)), "streaming threshold");
        std::map<uint64_t, std::set<int>> where;
        std::map<uint64_t, int> held;
        if (C.small) {
            seen.streamed++;
            CHECK(C.class_h.size() == C.class_groups.size(), "class lists");
            for (size_t k = 0; k < C.class_h.size(); ++k) {
                CHECK(k == 0 || C.class_h[k] > C.class_h[k - 1], "classes not ascending");
                if (C.class_h[k]) seen.above_chunk++;
                for (int g = C.class_groups[k].first; g < C.class_groups[k].second; ++g) {
                    CHECK(C.groups[g].x < csize && C.groups[g].t0 <= C.groups[g].t1 && C.groups[g].t1 <= (int)C.terms.size(), "streaming group");
                    where[C.groups[g].x | (C.class_h[k] << m)].insert((int)k);
                    held[C.groups[g].x | (C.class_h[k] << m)] += C.groups[g].t1 - C.groups[g].t0;
                }
            }
        } else {
            seen.tiled++;
            CHECK(C.M == std::min(REAL ? 13 : 12, m), "tile bits");
            seen.bits[C.M]++;
            if (C.passes.size() > 1) seen.multi_pass++;
            for (size_t pi = 0; pi < C.passes.size(); ++pi) {
                const TilePass &ps = C.passes[pi];
                const uint64_t S = REAL ? (ps.smask << 1) | 1ull : ps.smask;
                CHECK(__builtin_popcountll(S) == C.M && !(S >> m) && !(ps.d_out & S) && (ps.mask_lo | ps.mask_hi) == ps.smask &&
                          !(ps.mask_lo & ps.mask_hi) && (ps.mask_lo == 0 || ps.mask_hi == 0 || ps.mask_hi > ps.mask_lo) &&
                          __builtin_popcountll(ps.mask_lo) == std::min(TILE_EXPECT_LOG_NT, __builtin_popcountll(ps.smask)) && ps.d_out < shard,
                      "pass masks");
                CHECK(ps.a1 > ps.a0, "empty pass");
                if (ps.d_out >> m) seen.above_chunk++;
                if (ps.a1 - ps.a0 > 1) seen.multi_chunk++;
                // ket tile -> output tile over all chunks of the shard: a bijection of the shard's tiles
                std::set<uint64_t> outs;
                for (uint64_t c = 0; c < (shard >> m); ++c)
                    for (uint64_t tl = 0; tl < (csize >> C.M); ++tl) {
                        const uint64_t tb = REAL ? tile_base(tl, ps.smask) << 1 : tile_base(tl, ps.smask);
                        const uint64_t ob = ((c << m) | tb) ^ ps.d_out;
                        CHECK(tb < csize && !(tb & S) && ob < shard && !(ob & S), "tile base");
                        outs.insert(ob);
                    }
                CHECK(outs.size() == (shard >> C.M), "ket tile -> output tile is no bijection");
                for (int ch = ps.a0; ch < ps.a1; ++ch) {
                    const ExChunkT &ck = C.achunks[ch];
                    CHECK(ck.g1 - ck.g0 >= 1 && ck.g1 - ck.g0 <= TILE_APPLY_GROUPS && ck.t1 - ck.t0 <= TILE_TERM_CAP, "chunk caps");
                    CHECK(ch == ps.a0 || (ck.g0 == C.achunks[ch - 1].g1 && ck.t0 == C.achunks[ch - 1].t1), "chunks not contiguous");
                    if (ck.g1 - ck.g0 == TILE_APPLY_GROUPS) seen.group_cap++;
                    for (int g = ck.g0; g < ck.g1; ++g) {
                        const ExAGroupT &ag = C.agroups[g];
                        CHECK(ag.t0 >= ck.t0 && ag.t1 <= ck.t1 && ag.t0 <= ag.t1 && ag.x < (1u << C.M), "piece outside its chunk");
                        bool all_real = true;
                        for (int t = ag.t0; t < ag.t1; ++t) all_real = all_real && C.aterms[t].ci == 0.0;
                        CHECK((ag.pad & 1) == (all_real ? 1 : 0) && (!drop || all_real), "pad bit 0 / dropped terms");
                        const uint64_t x = spread(ag.x, S) | ps.d_out;
                        if (where[x].count((int)pi)) seen.cut++;   // (a further piece of a group that was cut)
                        where[x].insert((int)pi);
                        held[x] += ag.t1 - ag.t0;
                    }
                }
            }
        }
        CHECK(where.size() == want.size(), "groups of the tables %zu != groups %zu", where.size(), want.size());
        for (const auto &w : where)
            CHECK(want.count(w.first) && w.second.size() == 1 && held[w.first] == want[w.first], "a group in %zu passes / terms %d", w.second.size(),
                  held[w.first]);
        // --- the replay
        const uint64_t krank = rank ^ d;
        const cplx *bra = &phi[rank << nl];
        cplx *out = &sigma[rank << nl];
        for (uint64_t c = 0; c < (shard >> m); ++c) {
            const uint64_t ket_gbase = (krank << nl) | (c << m);
            const cplx *ket = &psi[ket_gbase];
            if (C.small) {
                for (size_t k = 0; k < C.class_h.size(); ++k) {
                    const uint64_t boff = (c ^ C.class_h[k]) << m;
                    CHECK(boff + csize <= shard, "output chunk beyond the shard");
                    for (uint64_t i = 0; i < csize; ++i) {
                        cplx s = 0.0;
                        for (int g = C.class_groups[k].first; g < C.class_groups[k].second; ++g) {
                            const uint64_t j = i ^ C.groups[g].x;
                            cplx D = 0.0;
                            for (int t = C.groups[g].t0; t < C.groups[g].t1; ++t)
                                D += cplx(C.terms[t].cr, REAL ? 0.0 : C.terms[t].ci) * psign((ket_gbase | j) & C.terms[t].z);
                            s += D * ket[j];
                        }
                        dot += std::conj(bra[boff + i]) * s;
                        out[boff + i] += s;
                    }
                }
                continue;
            }
            const uint32_t nel = 1u << C.M;
            std::vector<cplx> acc(nel);
            for (const TilePass &ps : C.passes) {
                // address of tile-local amplitude e inside its tile: the thread's share by mask_lo, the trip's by mask_hi; the real flavour
                // walks amplitude PAIRS (16-byte elements), bit 0 of e being the half of the pair
                auto pos = [&](uint32_t e) -> uint64_t {
                    const uint32_t el = REAL ? e >> 1 : e;
                    const uint64_t p = spread(el & (NT - 1), ps.mask_lo) | spread(el >> TILE_EXPECT_LOG_NT, ps.mask_hi);
                    return REAL ? (p << 1) | (e & 1u) : p;
                };
                for (uint64_t tl = 0; tl < (csize >> C.M); ++tl) {
                    const uint64_t tbv = tile_base(tl, ps.smask);                                  // (REAL: pair-index space)
                    const uint64_t tb = REAL ? tbv << 1 : tbv;
                    const uint64_t gbase = ket_gbase | tb;
                    const uint64_t ob = REAL ? ((((c << m) >> 1) | tbv) ^ (ps.d_out >> 1)) << 1 : ((c << m) | tbv) ^ ps.d_out;
                    std::fill(acc.begin(), acc.end(), cplx(0.0));
                    for (int ch = ps.a0; ch < ps.a1; ++ch) {
                        const ExChunkT &ck = C.achunks[ch];
                        for (int g = ck.g0; g < ck.g1; ++g) {
                            const ExAGroupT &ag = C.agroups[g];
                            for (uint32_t e = 0; e < nel; ++e) {
                                const uint32_t je = e ^ ag.x;
                                cplx D = 0.0;
                                for (int t = ag.t0; t < ag.t1; ++t)
                                    D += cplx(C.aterms[t].cr, REAL ? 0.0 : C.aterms[t].ci) * psign(gbase & C.aterms[t].zout) * psign(je & C.aterms[t].zin);
                                acc[e] += D * ket[tb | pos(je)];
                            }
                        }
                    }
                    for (uint32_t e = 0; e < nel; ++e) {
                        CHECK((ob | pos(e)) < shard, "output index beyond the shard");
                        dot += std::conj(bra[ob | pos(e)]) * acc[e];
                        out[ob | pos(e)] += acc[e];
                    }
                }
            }
        }
    }
}

int main(int argc, char **argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 200;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    std::normal_distribution<double> gauss;
    auto rnd = [&](uint64_t n) { return n ? rng() % n : 0; };
    Seen seen;
    for (int cs = 0; cs < cases; ++cs) {
        // (most cases small; every eighth one large enough for several tiles per chunk)
        const int nl = (cs % 8 == 0) ? 11 + (int)rnd(4) : ((cs & 1) ? 4 + (int)rnd(6) : 10 + (int)rnd(3));
        const int g = (nl >= 13) ? (int)rnd(2) : (int)rnd(4);
        const int n = nl + g;
        const int m = (cs % 3 == 0) ? nl : (cs % 3 == 1 ? std::max(2, nl - 1 - (int)rnd(2)) : 2 + (int)rnd(nl - 1));
        const uint64_t dim = 1ull << n, all = dim - 1;
        // style 0: real-symmetric (real coefficients, every string an even number of Y); 1: real coefficients, any number of Y;
        // 2: complex coefficients
        const int style = (cs / 2) % 3, kind = cs % 6;
        Sum H;
        auto add = [&](uint64_t x, uint64_t z) {
            if (style == 0 && (__builtin_popcountll(x & z) & 1)) z ^= x & (0ull - x);
            H.term(x, z, gauss(rng), style == 2 && rnd(2) ? gauss(rng) : 0.0);
        };
        auto low_x = [&]() { return rnd(1ull << std::min(n, 5)) | (rnd(3) == 0 ? rnd(dim) : 0); };
        std::vector<uint64_t> xs(3 + rnd(10));
        for (uint64_t &x : xs) x = low_x();
        const int nrand = 10 + (int)rnd(30);
        for (int t = 0; t < nrand; ++t) add(xs[rnd(xs.size())], rnd(dim));
        for (int t = 0; t < 4; ++t) add(0, rnd(dim));                                       // the diagonal group
        for (int t = 0; t < 6; ++t) add(rnd(dim), rnd(dim));                                // x anywhere: rank bits, above the chunk, low
        add(all, all), add(1ull << (n - 1), 0), add(1ull << (nl - 1), 1), add((1ull << (nl - 1)) | 3, rnd(dim));
        if ((kind == 1 || kind == 4) && n <= 13) {   // a group of more terms than TILE_TERM_CAP: cut into pieces
            const uint64_t xb = 5 | (g ? 1ull << nl : 0);
            for (int t = 0; t < TILE_TERM_CAP + 18; ++t) add(xb, rnd(dim));
        }
        if (kind == 2 && n <= 14) {   // more groups in one pass than TILE_APPLY_GROUPS
            for (int t = 0; t < 400; ++t) add(rnd(256) & all, rnd(dim));
        }
        const int64_t T = (int64_t)H.x.size();
        ByD by_d;
        double l1 = 0.0;
        for (int64_t t = 0; t < T; ++t) {
            HTerm ht;
            ht.z = H.z[t];
            fold_iny(H.cr[t], H.ci[t], __builtin_popcountll(H.x[t] & H.z[t]), ht.cr, ht.ci);
            RawGroup &gr = by_d[H.x[t] >> nl][H.x[t] & ((1ull << nl) - 1ull)];
            gr.x = H.x[t] & ((1ull << nl) - 1ull);
            gr.terms.push_back(ht);
            l1 += std::abs(cplx(H.cr[t], H.ci[t]));
        }
        for (int real = 0; real < 2; ++real) {
            if (real && style == 2) continue;   // (complex coefficients leave the real vectors)
            std::vector<cplx> psi(dim), phi(dim);
            double n2a = 0.0, n2b = 0.0;
            for (uint64_t i = 0; i < dim; ++i) {
                psi[i] = cplx(gauss(rng), real ? 0.0 : gauss(rng));
                phi[i] = cplx(gauss(rng), real ? 0.0 : gauss(rng));
                if (rnd(4) == 0) psi[i] = 0.0;
                n2a += std::norm(psi[i]), n2b += std::norm(phi[i]);
            }
            for (uint64_t i = 0; i < dim; ++i) psi[i] /= std::sqrt(n2a), phi[i] /= std::sqrt(n2b);
            cplx dot = 0.0, dot_ref = 0.0;
            std::vector<cplx> sigma(dim, 0.0), sigma_ref(dim, 0.0);
            for (uint64_t r = 0; r < (1ull << g); ++r) {
                if (real) replay_rank<true>(nl, r, by_d, m, true, psi, phi, dot, sigma, seen);
                else replay_rank<false>(nl, r, by_d, m, false, psi, phi, dot, sigma, seen);
            }
            const cplx iy[4] = {cplx(1, 0), cplx(0, 1), cplx(-1, 0), cplx(0, -1)};
            for (int64_t t = 0; t < T; ++t) {
                const cplx c = cplx(H.cr[t], H.ci[t]) * iy[__builtin_popcountll(H.x[t] & H.z[t]) & 3];
                for (uint64_t j = 0; j < dim; ++j) sigma_ref[j ^ H.x[t]] += c * psign(j & H.z[t]) * psi[j];
            }
            for (uint64_t i = 0; i < dim; ++i) dot_ref += std::conj(phi[i]) * sigma_ref[i];
            const double tol = 1e-12 * std::max(1.0, l1);
            // real flavour, odd-Y strings: their (imaginary) part of <phi|H|psi> is not computed; sigma would leave the real vectors
            const double derr = (real && style == 1) ? std::abs(dot.real() - dot_ref.real()) : std::abs(dot - dot_ref);
            CHECK(derr <= tol && (!real || dot.imag() == 0.0), "case %d flavour %d DOT: %.3e (nl %d g %d m %d style %d)", cs, real, derr, nl, g, m, style);
            if (!(real && style == 1)) {
                double worst = 0.0;
                for (uint64_t i = 0; i < dim; ++i) worst = std::max(worst, std::abs(sigma[i] - sigma_ref[i]));
                CHECK(worst <= tol, "case %d flavour %d APPLY: %.3e (nl %d g %d m %d style %d)", cs, real, worst, nl, g, m, style);
            }
        }
    }
    {   // a pass that can take no group is reported, not looped on: no input reaches it (pick_pass always leaves a taker), so only the
        // empty cover is checked here
        Cover C;
        CHECK(build_cover(C, {}, 12, false, false) && C.passes.empty() && !C.small && C.M == 12, "empty cover");
    }
    if (failures) return 1;
    std::printf("cross cover ok: %d cases, %d tiled covers (2^10: %d, 2^11: %d, 2^12: %d, 2^13: %d), %d streamed, %d with several passes, "
                "%d pieces of cut groups, %d passes of several chunks (%d chunks at the group cap), %d passes / classes above the chunk, "
                "%d groups with dropped terms\n",
                cases, seen.tiled, seen.bits[10], seen.bits[11], seen.bits[12], seen.bits[13], seen.streamed, seen.multi_pass, seen.cut,
                seen.multi_chunk, seen.group_cap, seen.above_chunk, seen.dropped);
    if (argc > 3) std::printf("hash %016llx\n", (unsigned long long)table_hash);
    return (seen.tiled && seen.streamed && seen.multi_pass && seen.cut && seen.multi_chunk && seen.group_cap && seen.above_chunk &&
            seen.dropped && seen.bits[10] && seen.bits[11] && seen.bits[12] && seen.bits[13])
               ? 0
               : 1;
}
