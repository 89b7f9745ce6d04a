// metric_plan_check.cpp — the host-side plan of the Fubini-Study metric (openvqe_amd/csrc/sv_metric_host.hpp) compiled alone with g++
// (ASan + UBSan in tests/test_metric_cases.py): random real rotation programs — plain same-x runs, runs fused into pattern tables the
// way the library fuses them, constant angles, offsets, tied and unused parameters — are restated on their compact support, the
// tangent kernel's loop is replayed on the host exactly as k_sparse_metric indexes its tables (every access bounds-checked), and the
// tangents are compared with a dense complex forward-mode simulation of exp(-i phi P).  Then the tangent store is laid out and the Gram
// schedule replayed the way k_rdm_gram / k_rdm_finish index it, against the plain Gram matrix.
//   usage: metric_plan_check [seed]
//          metric_plan_check boundary      the programs at the limits of the compact path: a support of exactly MAX_SUPPORT states
//                                          (compact index 4095 in the 12-bit fields of the pair words) with 20, 21, 3669 and 3670
//                                          rotations — the last program whose tables are staged in LDS, the first whose tables stay in
//                                          global memory, the last and the first beyond a workgroup's LDS budget — and the refusal at
//                                          the first state beyond the cap; prints the table sizes (tests/test_metric_cases.py)
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../../openvqe_amd/csrc/sv_metric_host.hpp"

using namespace ovqe;
using cd = std::complex<double>;

static int fails = 0, fused_ops = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            if (++fails > 20) std::exit(1);               \
        }                                                 \
    } while (0)

struct Rot {
    uint64_t x, z;
    double coeff, phi0;
    int pidx;
};

// (P a)_i = i^ny (-1)^{parity((i ^ x) & z)} a_{i ^ x}
static std::vector<cd> pauli(const std::vector<cd> &a, uint64_t x, uint64_t z) {
    const cd ph[4] = {cd(1, 0), cd(0, 1), cd(-1, 0), cd(0, -1)};
    const cd f = ph[__builtin_popcountll(x & z) & 3];
    std::vector<cd> out(a.size());
    for (uint64_t i = 0; i < a.size(); ++i) out[i] = f * (metric::parity64((i ^ x) & z) ? -1.0 : 1.0) * a[i ^ x];
    return out;
}
static void rotate(std::vector<cd> &a, uint64_t x, uint64_t z, double phi) {
    const std::vector<cd> p = pauli(a, x, z);
    for (size_t i = 0; i < a.size(); ++i) a[i] = std::cos(phi) * a[i] - cd(0, 1) * std::sin(phi) * p[i];
}

// the library's commuting-run fusion (try_table_op): patterns over the non-pivot x bits, K_e = sum_t -(-1)^{parity(ibits & z_t)} c_t
static bool fuse(const std::vector<Rot> &run, std::vector<metric::InRot> &rots, metric::InOp &op) {
    const uint64_t x = run[0].x, zc = run[0].z & ~x;
    const int w = __builtin_popcountll(x);
    if (w > 7 || run[0].pidx < 0) return false;
    for (const Rot &r : run)
        if (r.pidx != run[0].pidx || r.phi0 != 0.0 || (r.z & ~x) != zc) return false;
    int pos[8], np = 0;
    for (int b = 0; b < 64; ++b)
        if ((x >> b) & 1) pos[np++] = b;
    op = metric::InOp{x, zc, metric::KIND_TAB, (int)rots.size(), 0};
    for (uint32_t e = 0; e < (1u << (w - 1)); ++e) {
        uint64_t ibits = 0;
        for (int f = 0; f < w - 1; ++f)
            if ((e >> f) & 1) ibits |= 1ull << pos[f];
        double K = 0.0;
        for (const Rot &r : run) {
            double c = (__builtin_popcountll(r.x & r.z) & 2) ? -r.coeff : r.coeff;
            if (!metric::parity64(ibits & r.z)) c = -c;
            K += c;
        }
        if (K == 0.0) continue;
        rots.push_back(metric::InRot{ibits, K, 0.0, run[0].pidx, 1});
        op.count++;
    }
    return true;
}

static bool check_program(std::mt19937_64 &rng, int n, uint64_t hf, const std::vector<Rot> &prog, const std::vector<double> &theta, int K,
                          bool fuse_runs, metric::Compact *out);

static void one_program(std::mt19937_64 &rng, int n, int R, int K, bool fuse_runs) {
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    const uint64_t N = 1ull << n;
    const uint64_t hf = rng() & (N - 1);
    // a small family of x masks so that supports stay compact and same-x runs occur
    std::vector<uint64_t> xs;
    for (int k = 0; k < 3; ++k) {
        uint64_t x = 0;
        while (__builtin_popcountll(x) != 2 * (1 + k % 2)) x = rng() & (N - 1);
        xs.push_back(x);
    }
    std::vector<Rot> prog;
    for (int r = 0; r < R; ++r) {
        Rot q;
        q.x = (r && (rng() & 1)) ? prog.back().x : xs[rng() % xs.size()];
        for (;;) {   // an odd number of Y
            q.z = rng() & (N - 1);
            if (__builtin_popcountll(q.x & q.z) & 1) break;
        }
        q.pidx = (rng() % 7 == 0) ? -1 : (int)(rng() % (uint64_t)std::max(K - 1, 1));   // (the last parameter stays unused)
        q.coeff = U(rng);
        q.phi0 = (rng() % 3 == 0 || q.pidx < 0) ? U(rng) : 0.0;
        if (r && q.x == prog.back().x && (rng() & 1)) {   // the strings of one excitation: same parameter, same z outside x
            q.pidx = prog.back().pidx;
            q.z = (q.z & q.x) | (prog.back().z & ~q.x);
            if (!(__builtin_popcountll(q.x & q.z) & 1)) q.z ^= q.x & (~q.x + 1);
            q.phi0 = prog.back().phi0;
        }
        prog.push_back(q);
    }
    std::vector<double> theta((size_t)K);
    for (double &t : theta) t = U(rng);
    metric::Compact C;
    CHECK(check_program(rng, n, hf, prog, theta, K, fuse_runs, &C), "build_compact declined a real program (n = %d)", n);
}

// false: build_compact declined the program
static bool check_program(std::mt19937_64 &rng, int n, uint64_t hf, const std::vector<Rot> &prog, const std::vector<double> &theta, int K,
                          bool fuse_runs, metric::Compact *out) {
    const uint64_t N = 1ull << n;
    metric::Compact &C = *out;
    // ---- the fused-kernel program: same-x runs, fused where the structure allows
    std::vector<metric::InOp> ops;
    std::vector<metric::InRot> rots;
    for (size_t r = 0; r < prog.size();) {
        size_t e = r + 1;
        while (e < prog.size() && prog[e].x == prog[r].x) ++e;
        std::vector<Rot> run(prog.begin() + (long)r, prog.begin() + (long)e);
        metric::InOp op;
        if (fuse_runs && fuse(run, rots, op)) {
            if (op.count > 0) ops.push_back(op);
            ++fused_ops;
        } else {
            op = metric::InOp{prog[r].x, 0, metric::KIND_ROT, (int)rots.size(), (int)run.size()};
            for (const Rot &q : run) rots.push_back(metric::InRot{q.z, q.coeff, q.phi0, q.pidx, (int)(__builtin_popcountll(q.x & q.z) & 3)});
            ops.push_back(op);
        }
        r = e;
    }
    if (!metric::build_compact(hf, ops, rots, K, &C)) return false;
    CHECK(C.m >= 1 && C.m <= metric::MAX_SUPPORT && (int)C.first_op.size() == K, "shape");
    // ---- dense forward mode
    std::vector<cd> psi(N, 0.0);
    psi[hf] = 1.0;
    std::vector<std::vector<cd>> T((size_t)K, std::vector<cd>(N, 0.0));
    for (const Rot &q : prog) {
        const double phi = q.phi0 + (q.pidx >= 0 ? q.coeff * theta[(size_t)q.pidx] : 0.0);
        rotate(psi, q.x, q.z, phi);
        for (auto &t : T) rotate(t, q.x, q.z, phi);
        if (q.pidx >= 0) {
            const std::vector<cd> p = pauli(psi, q.x, q.z);
            for (uint64_t i = 0; i < N; ++i) T[(size_t)q.pidx][i] += q.coeff * cd(0, -1) * p[i];
        }
    }
    // ---- the kernel's loop on the compact program.  The compact numbering is not mapped back to register indices: psi is compared
    // as a sorted list of amplitudes, the tangents through their Gram matrix
    const metric::Store st = metric::store_layout(C.m, K, true);
    CHECK(st.wpad % rdm::GRAM_BLOCK == 0 && st.wpad >= K && st.bytes == (size_t)C.m * st.wpad * 8, "store layout");
    std::vector<double> store((size_t)C.m * st.wpad, 0.0);
    const int nops = (int)C.ops.size(), ntab = (int)C.tab.size();
    std::vector<double> psi_c;
    for (int k = 0; k < K; ++k) {
        std::vector<double> a((size_t)C.m, 0.0), t((size_t)C.m, 0.0), c((size_t)ntab), s((size_t)ntab), dk((size_t)ntab);
        a.at((size_t)C.hf) = 1.0;
        for (int e = 0; e < ntab; ++e) {
            const metric::TabEntry &te = C.tab[(size_t)e];
            const double phi = te.phi0 + (te.pidx >= 0 ? te.coeff * theta.at((size_t)te.pidx) : 0.0);
            c[(size_t)e] = std::cos(phi);
            s[(size_t)e] = std::sin(phi);
            dk[(size_t)e] = te.pidx == k ? te.coeff : 0.0;
        }
        const int o1 = std::min(C.first_op.at((size_t)k), nops);
        for (int o = 0; o < nops; ++o) {
            const metric::Op &op = C.ops[(size_t)o];
            std::vector<char> touched((size_t)C.m, 0);
            for (int pe = 0; pe < op.npairs; ++pe) {
                const uint32_t pw = C.pairs.at((size_t)(op.first + pe));
                const uint32_t ci = pw & 0xfffu, cj = (pw >> 12) & 0xfffu;
                const size_t e = (size_t)op.tab0 + (pw >> 25);
                CHECK(e < (size_t)ntab && ci < (uint32_t)C.m && cj < (uint32_t)C.m && ci != cj, "pair word out of range");
                CHECK(!touched[ci] && !touched[cj], "the pairs of one op are not disjoint");
                touched[ci] = touched[cj] = 1;
                const bool neg = (pw >> 24) & 1u;
                const double sn = neg ? -s.at(e) : s.at(e), d = neg ? -dk.at(e) : dk.at(e);
                if (o < o1) CHECK(d == 0.0, "first_op skips an op that holds an entry of parameter %d", k);
                const double u = a[ci], v = a[cj], tu = t[ci], tv = t[cj];
                const double u1 = c[e] * u + sn * v, v1 = c[e] * v - sn * u;
                a[ci] = u1;
                a[cj] = v1;
                if (o >= o1) {
                    t[ci] = c[e] * tu + sn * tv + d * v1;
                    t[cj] = c[e] * tv - sn * tu - d * u1;
                }
            }
        }
        for (int i = 0; i < C.m; ++i) store.at((size_t)i * st.wpad + (size_t)k) = t[(size_t)i];
        psi_c = a;
    }
    // psi: same multiset of amplitudes, no imaginary part
    {
        std::vector<double> d, cidx(psi_c);
        for (const cd &v : psi) {
            CHECK(std::fabs(v.imag()) < 1e-13, "dense psi has an imaginary part");
            if (std::fabs(v.real()) > 1e-14) d.push_back(v.real());
        }
        std::vector<double> cc;
        for (double v : cidx)
            if (std::fabs(v) > 1e-14) cc.push_back(v);
        std::sort(d.begin(), d.end());
        std::sort(cc.begin(), cc.end());
        CHECK(d.size() == cc.size(), "support of psi: %zu dense, %zu compact", d.size(), cc.size());
        for (size_t i = 0; i < std::min(d.size(), cc.size()); ++i) CHECK(std::fabs(d[i] - cc[i]) < 1e-12, "psi amplitude %zu", i);
    }
    // ---- Gram matrix through the schedule, the way k_rdm_gram / k_rdm_finish index store and slabs
    const rdm::Schedule S = metric::gram_plan(st, 1 + (int)(rng() % 300));
    CHECK(S.slices >= 1 && S.slice_rows % S.tile_rows == 0 && (int64_t)S.slices * S.slice_rows >= st.rows, "Gram schedule");
    CHECK(S.slab_elems == (size_t)S.npairs * S.slices * 64 * 64, "slab size");
    std::vector<double> slabs(S.slab_elems, 0.0);
    for (int b = 0; b < S.npairs * S.slices; ++b) {
        const int pair = b / S.slices, slice = b - pair * S.slices;
        const int64_t r0 = (int64_t)slice * S.slice_rows, r1 = std::min<int64_t>(r0 + S.slice_rows, st.rows);
        int I, J;
        rdm::block_pair(pair, S.nblk, &I, &J);
        CHECK(I <= J && J < S.nblk && rdm::block_pair_index(I, J, S.nblk) == pair, "block pair");
        for (int64_t r = r0; r < r1; ++r)
            for (int p = 0; p < 64; ++p)
                for (int q = 0; q < 64; ++q)
                    slabs.at((size_t)b * 4096 + (size_t)p * 64 + (size_t)q) +=
                        store.at((size_t)r * st.wpad + (size_t)I * 64 + p) * store.at((size_t)r * st.wpad + (size_t)J * 64 + q);
    }
    double worst = 0.0, scale = 1.0;
    for (int p = 0; p < K; ++p)
        for (int q = p; q < K; ++q) {
            const int I = p / 64, J = q / 64;
            double g = 0.0;
            for (int s = 0; s < S.slices; ++s)
                g += slabs.at(((size_t)rdm::block_pair_index(I, J, S.nblk) * S.slices + (size_t)s) * 4096 + (size_t)(p - I * 64) * 64 + (size_t)(q - J * 64));
            cd tt = 0.0, tp = 0.0, tq = 0.0;
            for (uint64_t i = 0; i < N; ++i) {
                tt += std::conj(T[(size_t)p][i]) * T[(size_t)q][i];
                tp += std::conj(T[(size_t)p][i]) * psi[i];
                tq += std::conj(T[(size_t)q][i]) * psi[i];
            }
            CHECK(std::abs(tp) < 1e-12, "<T|psi> of a real program");
            const double want = (tt - tp * std::conj(tq)).real();
            if (p == q) scale = std::max(scale, want);
            worst = std::max(worst, std::fabs(g - want));
        }
    CHECK(worst <= 1e-12 * scale, "metric differs from the dense simulation by %.3e (n = %d, K = %d, fused = %d)", worst, n, K, (int)fuse_runs);
    if (K >= 1) {   // the unused last parameter: a zero column
        bool used = false;
        for (const Rot &q : prog) used = used || q.pidx == K - 1;
        for (int i = 0; i < C.m; ++i) CHECK(used || store[(size_t)i * st.wpad + (size_t)(K - 1)] == 0.0 || K == 1, "unused parameter");
    }
    return true;
}

// ---- boundary mode ------------------------------------------------------------------------------------------------------------------
// the tangent kernel's dynamic LDS is sp_metric_lds itself (sv_sparse_layout.hpp: the header the kernel and its launcher read)
constexpr size_t LDS_BUDGET = 150 * 1024, LDS_MAX = 160 * 1024;   // LDS_WG_BUDGET / LDS_WG_MAX of ovqe_sv.hip

// cube program: a single Y on bit r for r < n (the support doubles up to the whole register), then odd-Y strings of weight 2..5; every
// rotation with an offset, so that none is fused; pidx from -1..K-1
static std::vector<Rot> cube_program(std::mt19937_64 &rng, int n, int R, int K) {
    std::uniform_real_distribution<double> U(0.2, 1.0);
    std::vector<Rot> prog;
    const double scale = std::min(0.6, 1.2 / std::sqrt((double)R / (K + 1)));
    for (int r = 0; r < R; ++r) {
        Rot q{0, 0, 0, 0, 0};
        if (r < n) {
            q.x = q.z = 1ull << (n - 1 - r);
        } else {
            for (;;) {
                q.x = q.z = 0;
                const int w = 2 + (int)(rng() % 4);
                while (__builtin_popcountll(q.x | q.z) < w) {
                    const uint64_t bit = 1ull << (rng() % (uint64_t)n);
                    if ((q.x | q.z) & bit) continue;
                    const int letter = (int)(rng() % 3);   // X, Y, Z
                    if (letter != 2) q.x |= bit;
                    if (letter != 0) q.z |= bit;
                }
                if (__builtin_popcountll(q.x & q.z) & 1) break;
            }
        }
        q.pidx = r <= K ? r - 1 : (int)(rng() % (uint64_t)(K + 1)) - 1;
        q.coeff = ((rng() & 1) ? scale : -scale) * (0.1 + U(rng));
        q.phi0 = ((rng() & 1) ? 1.0 : -1.0) * U(rng);
        prog.push_back(q);
    }
    return prog;
}

static void boundary() {
    std::mt19937_64 rng(12);
    std::uniform_real_distribution<double> U(-0.8, 0.8);
    std::vector<double> theta(6);
    for (double &t : theta) t = U(rng);
    for (int R : {20, 21, 3669, 3670}) {
        const int n = 12, K = R < 100 ? 6 : 2;   // (the long programs with two parameters: the replay and the dense simulation cost R K 2^n)
        const std::vector<Rot> prog = cube_program(rng, n, R, K);
        metric::Compact C;
        const bool ok = check_program(rng, n, rng() & ((1ull << n) - 1), prog, theta, K, true, &C);   // (fusion on: the offsets refuse it)
        CHECK(ok, "build_compact declined the cube program n = %d R = %d", n, R);
        if (!ok) continue;
        uint32_t max_ci = 0, max_cj = 0;
        for (const uint32_t pw : C.pairs) {
            max_ci = std::max(max_ci, pw & 0xfffu);
            max_cj = std::max(max_cj, (pw >> 12) & 0xfffu);
            CHECK((pw >> 25) == 0, "a plain op with a pattern");
        }
        CHECK(C.m == metric::MAX_SUPPORT && max_cj == 4095u, "m = %d, max cj = %u", C.m, max_cj);
        CHECK((int)C.tab.size() == R && (int)C.ops.size() == R, "one op and one table entry per rotation: %zu, %zu", C.ops.size(), C.tab.size());
        // the LDS regions the kernel indexes: psi / t by ci, cj < mpad, cs / dk by e < ntab, the op records and pair words when staged
        const SpMetricArgs A = sp_metric_args(C, K);
        const SpMetricLds Ls = sp_metric_lds(A, true), Lu = sp_metric_lds(A, false);
        const int form = Ls.bytes <= LDS_BUDGET ? 1 : Lu.bytes <= LDS_BUDGET ? 2 : 0;
        const SpMetricLds &L = form == 1 ? Ls : Lu;
        const size_t mpad = (size_t)((C.m + 1) & ~1);
        CHECK(((size_t)std::max(max_ci, max_cj) + 1) * 8 <= L.t && L.t + mpad * 8 <= L.cs, "psi / tangent region");
        CHECK(L.cs % 16 == 0 && L.cs + C.tab.size() * 16 <= L.dk && L.dk + C.tab.size() * 8 <= L.ops && L.ops % 16 == 0, "table regions");
        if (form == 1) CHECK(L.ops + C.ops.size() * 16 <= L.pairs && L.pairs + C.pairs.size() * 4 == L.bytes, "staged regions");
        if (form) CHECK(L.bytes <= LDS_BUDGET && L.bytes <= LDS_MAX, "the launch exceeds the budget");
        for (size_t o = 0; o < C.ops.size(); ++o)
            CHECK(C.ops[o].first >= 0 && (size_t)C.ops[o].first + (size_t)C.ops[o].npairs <= C.pairs.size() && C.ops[o].tab0 == (int)o, "op %zu", o);
        std::printf("cube n=%d R=%d ok=1 m=%d ntab=%zu nops=%zu npairs=%zu max_ci=%u max_cj=%u staged=%zu unstaged=%zu form=%d\n", n, R, C.m,
                    C.tab.size(), C.ops.size(), C.pairs.size(), max_ci, max_cj, Ls.bytes, Lu.bytes, form);
    }
    // one qubit more: the 13th Y rotation reaches state 4097 and build_compact declines, with or without rotations behind it
    const int K = 6;
    for (int R : {13, 21}) {
        const std::vector<Rot> prog = cube_program(rng, 13, R, K);
        metric::Compact C;
        const bool ok = check_program(rng, 13, 5, prog, theta, K, true, &C);
        CHECK(!ok, "a support of 8192 states accepted (R = %d)", R);
        std::printf("cube n=13 R=%d ok=%d\n", R, (int)ok);
    }
    // ... and the 12 Y rotations alone are accepted, at the cap
    {
        const std::vector<Rot> prog = cube_program(rng, 12, 12, K);
        metric::Compact C;
        CHECK(check_program(rng, 12, 77, prog, theta, K, true, &C) && C.m == metric::MAX_SUPPORT, "the cap itself declined");
    }
}

int main(int argc, char **argv) {
    if (argc > 1 && !std::strcmp(argv[1], "boundary")) {
        boundary();
        if (fails) {
            std::printf("metric plan: %d failures\n", fails);
            return 1;
        }
        std::printf("metric plan boundary ok\n");
        return 0;
    }
    std::mt19937_64 rng(argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1);
    const int Ks[] = {1, 2, 5, 63, 64, 65, 129};
    int programs = 0;
    for (int rep = 0; rep < 3; ++rep)
        for (int K : Ks)
            for (int fused = 0; fused < 2; ++fused) {
                const int n = 5 + (int)(rng() % 4);
                one_program(rng, n, std::max(6, K < 16 ? 24 : K + 8), K, fused != 0);
                ++programs;
            }
    // declined forms: a diagonal rotation, an even number of Y, a literal gate
    {
        metric::Compact C;
        std::vector<metric::InRot> rots = {metric::InRot{1, 0.3, 0.0, 0, 0}};
        CHECK(!metric::build_compact(0, {metric::InOp{0, 0, metric::KIND_ROT, 0, 1}}, rots, 1, &C), "diagonal rotation accepted");
        CHECK(!metric::build_compact(0, {metric::InOp{3, 0, metric::KIND_ROT, 0, 1}}, rots, 1, &C), "even-Y rotation accepted");
        CHECK(!metric::build_compact(0, {metric::InOp{1, 0, 3, 0, 0}}, rots, 1, &C), "literal gate accepted");
        CHECK(!metric::build_compact(0, {metric::InOp{1, 0, metric::KIND_ROT, 0, 2}}, rots, 1, &C), "table overrun accepted");
    }
    // the streaming store: psi in column 0, 16-byte amplitudes
    {
        const metric::Store st = metric::store_layout(1 << 14, 140, false);
        CHECK(st.width == 141 && st.wpad == 192 && st.bytes == (size_t)(1 << 14) * 192 * 16, "streaming store");
        const rdm::Schedule S = metric::gram_plan(st, 256);
        CHECK(S.tile_rows == 16 && S.nblk == 3 && S.npairs == 6 && (int64_t)S.slices * S.slice_rows >= st.rows, "streaming Gram schedule");
        const metric::Store big = metric::store_layout((int64_t)1 << 24, 1715, false);
        CHECK(big.bytes == ((size_t)1 << 24) * 1728 * 16, "N2 store bytes");
    }
    if (fails) {
        std::printf("metric plan: %d failures\n", fails);
        return 1;
    }
    CHECK(fused_ops > 0, "no run was fused");
    std::printf("metric plan ok (%d programs, %d fused runs)\n", programs, fused_ops);
    if (fails) return 1;
    return 0;
}
