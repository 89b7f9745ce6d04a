// pool_cover_check.cpp — the host-side planner of the ADAPT pool screen on the partitioned register (openvqe_amd/csrc/sv_pool_host.hpp)
// compiled alone with g++ (ASan + UBSan: tests/test_pool_cover.py).  For random registers (n_local 4..14, 0..3 rank bits, chunk bits
// from 2 up to n_local) and random pools the plan of every rank is replayed on the CPU the way k_tile_pool / k_tile_pool_real /
// k_pool_small index it — tile by tile, staged chunks, entry tables, signs from zin / zout, d_out pairing ket chunk c with bra
// chunk c ^ h, one partial row per workgroup of the grid-stride — and every v_k = sum_t c_t <sigma|P_t|psi> is compared with the
// term-by-term definition to 1e-12 max(1, |c_k|_1), for the complex and the real flavour.  Conditions on the tables: every
// (operator, x) entry lies in exactly one pass, passes per rank difference <= its distinct x masks, the staged chunks respect the
// caps, the partial storage depends on the operator count alone.
//   usage: pool_cover_check <cases> <seed> [hash]      (hash: also print one 64-bit hash over every table built)
#include "../../openvqe_amd/csrc/sv_pool_host.hpp"

#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

using namespace ovqe;
using namespace ovqe::pool;
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
    const int64_t head[8] = {(int64_t)C.d, C.m, C.small ? 1 : 0, C.M, C.n_entries, C.n_x, C.n_terms, 0};
    hash_bytes(head, sizeof head);
    hash_vec(C.passes), hash_vec(C.chunks), hash_vec(C.entries), hash_vec(C.terms), hash_vec(C.class_h), hash_vec(C.class_entries);
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

struct Pool {
    std::vector<int64_t> offsets{0};
    std::vector<uint64_t> x, z;
    std::vector<double> cr, ci;
    void term(uint64_t xx, uint64_t zz, double a, double b) {
        x.push_back(xx), z.push_back(zz), cr.push_back(a), ci.push_back(b);
    }
    void close() { offsets.push_back((int64_t)x.size()); }
    int64_t n_ops() const { return (int64_t)offsets.size() - 1; }
};

// one rank's screen from the plan tables, as the kernels run it -> v_k partial of that rank
template <bool REAL>
static void replay_rank(int nl, int g, uint64_t rank, const std::map<uint64_t, std::vector<RawEntry>> &by_d, int chunk_bits,
                        const std::vector<cplx> &psi, const std::vector<cplx> &sigma, int64_t n_ops, std::vector<cplx> &v,
                        const std::set<std::pair<int, uint64_t>> *all_entries_of_d0_check) {
    (void)g;
    (void)all_entries_of_d0_check;
    const uint64_t shard = 1ull << nl;
    std::vector<cplx> rows((size_t)POOL_ROWS * (size_t)std::max<int64_t>(n_ops, 1));
    CHECK(rows.size() * 16 == partial_bytes(n_ops), "partial bytes");
    for (const auto &kv : by_d) {
        const uint64_t d = kv.first;
        Cover C;
        C.d = d;
        const int m = d ? chunk_bits : nl;
        build_cover(C, kv.second, m, REAL);
        hash_cover(C);
        const uint64_t csize = 1ull << m;
        // --- conditions on the tables
        std::set<uint64_t> xs;
        std::set<std::pair<int, uint64_t>> want;
        for (const RawEntry &e : kv.second) xs.insert(e.x), want.insert({e.slot, e.x});
        CHECK(C.n_x == (int)xs.size() && C.n_entries == (int)kv.second.size(), "counts");
        CHECK(C.n_passes() <= (int64_t)xs.size(), "passes %lld > distinct x masks %zu", (long long)C.n_passes(), xs.size());
        CHECK(C.small == (m < (REAL ? 11 : 10)), "streaming threshold");
        std::map<std::pair<int, uint64_t>, std::set<int>> where;
        if (C.small) {
            for (size_t k = 0; k < C.class_h.size(); ++k)
                for (int e = C.class_entries[k].first; e < C.class_entries[k].second; ++e)
                    where[{C.entries[e].slot, (uint64_t)C.entries[e].x | (C.class_h[k] << m)}].insert((int)k);
        } else {
            CHECK(C.M == std::min(REAL ? 13 : 12, m), "tile bits");
            for (size_t pi = 0; pi < C.passes.size(); ++pi) {
                const auto &ps = C.passes[pi];
                const uint64_t S = REAL ? (ps.smask << 1) | 1ull : ps.smask;
                CHECK(__builtin_popcountll(S) == C.M && !(S >> m) && !(ps.d_out & S) && (ps.mask_lo | ps.mask_hi) == ps.smask &&
                          !(ps.mask_lo & ps.mask_hi) && __builtin_popcountll(ps.mask_lo) == std::min(TILE_EXPECT_LOG_NT, __builtin_popcountll(ps.smask)),
                      "pass masks");
                CHECK(ps.a1 > ps.a0, "empty pass");
                for (int ch = ps.a0; ch < ps.a1; ++ch) {
                    const auto &ck = C.chunks[ch];
                    CHECK(ck.g1 - ck.g0 >= 1 && ck.g1 - ck.g0 <= POOL_ENTRY_CAP && ck.t1 - ck.t0 <= POOL_TERM_CAP, "chunk caps");
                    int covered = 0;
                    for (int e = ck.g0; e < ck.g1; ++e) {
                        const PoolEntry &en = C.entries[e];
                        CHECK(en.t0 >= ck.t0 && en.t1 <= ck.t1 && en.t0 <= en.t1, "entry terms outside the chunk");
                        if (en.run > 0) {
                            CHECK(e == ck.g0 + covered, "runs overlap");
                            for (int r = e; r < e + en.run; ++r) CHECK(r < ck.g1 && C.entries[r].slot == en.slot, "run of another slot");
                            covered += en.run;
                        }
                        where[{en.slot, spread(en.x, S) | ps.d_out}].insert((int)pi);
                    }
                    CHECK(covered == ck.g1 - ck.g0, "runs do not cover the chunk");
                }
            }
        }
        CHECK(where.size() == want.size(), "entries of the tables %zu != (operator, x) pairs %zu", where.size(), want.size());
        for (const auto &w : where) CHECK(want.count(w.first) && w.second.size() == 1, "an entry in %zu passes", w.second.size());
        // --- the replay
        const uint64_t krank = rank ^ d;
        for (uint64_t c = 0; c < (shard >> m); ++c) {
            const cplx *ket = &psi[(krank << nl) | (c << m)];
            const cplx *bra = &sigma[rank << nl];
            const uint64_t ket_gbase = (krank << nl) | (c << m);
            if (C.small) {
                const uint64_t nb = std::min<uint64_t>(POOL_SMALL_ROWS, std::max<uint64_t>(1, (csize + 255) / 256));
                for (size_t k = 0; k < C.class_h.size(); ++k) {
                    const uint64_t boff = (c ^ C.class_h[k]) << m;
                    CHECK(boff + csize <= shard, "bra chunk beyond the shard");
                    for (int e = C.class_entries[k].first; e < C.class_entries[k].second; ++e) {
                        const PoolEntry &en = C.entries[e];
                        for (uint64_t i = 0; i < csize; ++i) {
                            const uint64_t j = i ^ en.x;
                            CHECK(j < csize, "ket index beyond the chunk");
                            cplx D = 0.0;
                            for (int t = en.t0; t < en.t1; ++t) D += cplx(C.terms[t].cr, C.terms[t].ci) * psign((ket_gbase | j) & C.terms[t].zout);
                            rows[((i / 256) % nb) * n_ops + en.slot] += std::conj(bra[boff + i]) * D * ket[j];
                        }
                    }
                }
                continue;
            }
            const uint64_t ntiles = csize >> C.M;
            const uint64_t grid = std::min<uint64_t>(ntiles, POOL_ROWS);
            for (const auto &ps : C.passes) {
                const uint64_t S = REAL ? (ps.smask << 1) | 1ull : ps.smask;
                for (uint64_t tl = 0; tl < ntiles; ++tl) {
                    uint64_t tb = tile_base(tl, ps.smask);   // (REAL: pair-index space)
                    if (REAL) tb <<= 1;
                    CHECK(tb < csize && !(tb & S), "tile base");
                    const uint64_t gbase = ket_gbase | tb;
                    const uint64_t ob = ((c << m) | tb) ^ ps.d_out;
                    CHECK(ob < shard && !(ob & S), "bra tile beyond the shard");
                    cplx *row = &rows[(tl % grid) * std::max<int64_t>(n_ops, 1)];
                    for (int ch = ps.a0; ch < ps.a1; ++ch) {
                        const auto &ck = C.chunks[ch];
                        for (int e = ck.g0; e < ck.g1; ++e) {
                            const PoolEntry &en = C.entries[e];
                            CHECK(en.x < (1u << C.M), "tile-local x");
                            cplx part = 0.0;
                            for (uint32_t i = 0; i < (1u << C.M); ++i) {
                                const uint32_t je = i ^ en.x;
                                cplx D = 0.0;
                                for (int t = en.t0; t < en.t1; ++t)
                                    D += cplx(C.terms[t].cr, C.terms[t].ci) * psign(gbase & C.terms[t].zout) * psign(je & C.terms[t].zin);
                                part += std::conj(bra[ob | spread(i, S)]) * D * ket[tb | spread(je, S)];
                            }
                            row[en.slot] += part;
                        }
                    }
                }
            }
        }
    }
    for (int64_t k = 0; k < n_ops; ++k)
        for (int r = 0; r < POOL_ROWS; ++r) v[k] += rows[(size_t)r * n_ops + k];
}

int main(int argc, char **argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 200;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    std::normal_distribution<double> gauss;
    auto rnd = [&](uint64_t n) { return n ? rng() % n : 0; };
    int tiled = 0, streamed = 0, multi_pass = 0;
    for (int cs = 0; cs < cases; ++cs) {
        // (most cases small; every eighth one large enough for several tiles per chunk)
        const int nl = (cs % 8 == 0) ? 11 + (int)rnd(4) : ((cs & 1) ? 4 + (int)rnd(6) : 10 + (int)rnd(3));
        const int g = (nl >= 13) ? (int)rnd(2) : (int)rnd(4);
        const int n = nl + g;
        const int m = (cs % 3 == 0) ? nl : (cs % 3 == 1 ? std::max(2, nl - 1 - (int)rnd(2)) : 2 + (int)rnd(nl - 1));
        const uint64_t dim = 1ull << n, all = dim - 1;
        Pool P;
        const int kind = cs % 6;
        const int nrand = 2 + (int)rnd(8);
        auto low_x = [&]() { return rnd(1ull << std::min(n, 5)) | (rnd(3) == 0 ? (rnd(dim)) : 0); };
        for (int k = 0; k < nrand; ++k) {
            const int nt = (int)rnd(5);
            const uint64_t x0 = low_x();
            for (int t = 0; t < nt; ++t) P.term(rnd(2) ? x0 : low_x(), rnd(dim), gauss(rng), rnd(2) ? gauss(rng) : 0.0);
            P.close();
        }
        {   // two operators sharing one x mask
            const uint64_t xs = low_x() | (1ull << (n - 1));
            P.term(xs, rnd(dim), 1.0, 0.5), P.close();
            P.term(xs, rnd(dim), -0.25, 0.0), P.term(xs, rnd(dim), 0.0, 2.0), P.close();
        }
        {   // an operator spread over several partners and several passes: x on the rank bits, above the chunk, and low
            for (int t = 0; t < 6; ++t) P.term(rnd(dim) & all, rnd(dim), gauss(rng), gauss(rng));
            P.term(all, all, 0.3, 0.0), P.term(1ull << (n - 1), 0, 0.0, -1.0), P.term(1ull << (nl - 1), 1, 1.0, 0.0);
            P.close();
        }
        P.term(0, rnd(dim), 0.7, 0.0), P.term(0, rnd(dim), 0.0, -0.2), P.close();   // a diagonal operator
        P.close();                                                                    // an operator with no terms
        if (kind == 1 && n <= 13) {   // more terms on one x than TILE_TERM_CAP (512): pieces that feed one accumulator
            const uint64_t xb = 5 | (g ? 1ull << nl : 0);
            for (int t = 0; t < 530; ++t) P.term(xb, rnd(dim), gauss(rng) / 530.0, gauss(rng) / 530.0);
            P.close();
        }
        if (kind == 2 && n <= 14) {   // more entries in a pass than the group cap
            for (int k = 0; k < 150; ++k) P.term(rnd(16), rnd(dim), gauss(rng), 0.0), P.close();
        }
        const int64_t n_ops = P.n_ops();
        std::map<uint64_t, std::vector<RawEntry>> by_d;
        const std::string err = collect(nl, n, n_ops, P.offsets.data(), P.x.data(), P.z.data(), P.cr.data(), P.ci.data(), by_d);
        CHECK(err.empty(), "collect: %s", err.c_str());
        for (int real = 0; real < 2; ++real) {
            std::vector<cplx> psi(dim), sigma(dim);
            double n2a = 0.0, n2b = 0.0;
            for (uint64_t i = 0; i < dim; ++i) {
                psi[i] = cplx(gauss(rng), real ? 0.0 : gauss(rng));
                sigma[i] = cplx(gauss(rng), real ? 0.0 : gauss(rng));
                if (rnd(4) == 0) psi[i] = 0.0;
                n2a += std::norm(psi[i]), n2b += std::norm(sigma[i]);
            }
            for (uint64_t i = 0; i < dim; ++i) psi[i] /= std::sqrt(n2a), sigma[i] /= std::sqrt(n2b);
            std::vector<cplx> v(n_ops, 0.0), ref(n_ops, 0.0);
            for (uint64_t r = 0; r < (1ull << g); ++r) {
                if (real) replay_rank<true>(nl, g, r, by_d, m, psi, sigma, n_ops, v, nullptr);
                else replay_rank<false>(nl, g, r, by_d, m, psi, sigma, n_ops, v, nullptr);
            }
            const cplx iy[4] = {cplx(1, 0), cplx(0, 1), cplx(-1, 0), cplx(0, -1)};
            for (int64_t k = 0; k < n_ops; ++k) {
                double l1 = 0.0;
                for (int64_t t = P.offsets[k]; t < P.offsets[k + 1]; ++t) {
                    const cplx c = cplx(P.cr[t], P.ci[t]) * iy[__builtin_popcountll(P.x[t] & P.z[t]) & 3];
                    l1 += std::abs(c);
                    cplx s = 0.0;
                    for (uint64_t j = 0; j < dim; ++j) s += std::conj(sigma[j ^ P.x[t]]) * psign(j & P.z[t]) * psi[j];
                    ref[k] += c * s;
                }
                CHECK(std::abs(v[k] - ref[k]) <= 1e-12 * std::max(1.0, l1), "case %d flavour %d op %lld: %.3e (nl %d g %d m %d)", cs, real,
                      (long long)k, std::abs(v[k] - ref[k]), nl, g, m);
            }
        }
        for (const auto &kv : by_d) {
            Cover C;
            build_cover(C, kv.second, kv.first ? m : nl, false);
            (C.small ? streamed : tiled)++;
            if (C.n_passes() > 1) ++multi_pass;
        }
    }
    // the refusals of collect()
    {
        std::map<uint64_t, std::vector<RawEntry>> by_d;
        const int64_t bad[3] = {0, 2, 1};
        const uint64_t x[2] = {1, 1ull << 9}, z[2] = {0, 0};
        const double c[2] = {1.0, 1.0};
        CHECK(!collect(4, 6, 2, bad, x, z, c, nullptr, by_d).empty(), "non-monotone offsets accepted");
        const int64_t good[3] = {0, 1, 2};
        CHECK(!collect(4, 6, 2, good, x, z, c, nullptr, by_d).empty(), "mask beyond the register accepted");
    }
    if (failures) return 1;
    std::printf("pool cover ok: %d cases, %d tiled covers, %d streamed, %d with several passes\n", cases, tiled, streamed, multi_pass);
    if (argc > 3) std::printf("hash %016llx\n", (unsigned long long)table_hash);
    return (tiled && streamed && multi_pass) ? 0 : 1;
}
